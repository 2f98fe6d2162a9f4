"""GPU tests of the stand-alone pivoted LU (clrsdp_getrf / solver.getrf, include/clrsdp.h): the
one-CU getrf_batched where its on-chip panel fits (fp64 n <= 624, double-double 312, quad-double
156) and the blocked chain across workgroups beyond (getrf_blk_panel / _swap / _update, also
forced at every size by CLRSDP_LU_BLK=1).

Probing residual: for v in {ones, two +-1 sketches}, r = A[perm, :] v - L (U v) in mpmath at 320
bits, against the a-priori bound gamma_n |L| |U| |v| with a margin of 8:
|r_i| <= 8 n eps (|L| (|U| |v|))_i, eps = 2^-53 / 2^-104 / 2^-206.  The largest ratio to that
bound is printed by every test (measured: DESIGN.md section 3).
"""
import mpmath
import numpy as np
import pytest

from helpers import sketch_weights

pytestmark = pytest.mark.gpu

EPS = {1: 2.0 ** -53, 2: 2.0 ** -104, 4: 2.0 ** -206}
BOUND = {1: 624, 2: 312, 4: 156}     # the largest n of the one-CU kernel
PREC = 320
_mpf = np.frompyfunc(mpmath.mpf, 1, 1)


def _matrix(pk, n, words, kind, seed=11):
    """float limb terms (words > 1: three of them, so the entries are genuinely wide) of
    kind 0: random non-symmetric; 1: the same with row i scaled by 2^-(i mod 40);
    2: 0.01 random + 4 (reversed identity) -- every pivot comes from far below the panel."""
    from clrsdp_amd import instance as inst
    terms = []
    for t in range(1 if words == 1 else 3):
        u = inst.uniform(seed + 7 * kind, 500 + t, n * n).reshape(n, n) * 2.0 ** (-53 * t)
        if kind == 1:
            u = u * (2.0 ** -(np.arange(n) % 40))[:, None]
        if kind == 2:
            u = 0.01 * u
            if t == 0:
                u = u + 4.0 * np.eye(n)[::-1]
        terms.append(u)
    return terms


def _block(terms):
    """the exact sum of the limb terms: a float array (one term) or mpf objects"""
    if len(terms) == 1:
        return terms[0]
    with mpmath.workprec(PREC):
        A = _mpf(terms[0])
        for t in terms[1:]:
            A = A + _mpf(t)
    return A


def _exact(limbs):
    """(words, n, n) float limbs -> their exact sums as mpf objects"""
    with mpmath.workprec(PREC):
        A = _mpf(limbs[0])
        for t in limbs[1:]:
            A = A + _mpf(t)
    return A


def probe_ratio(A, LUl, perm, words):
    """max_i |r_i| / (8 n eps (|L| (|U| |v|))_i) over the three probing vectors."""
    n = A.shape[0]
    assert sorted(int(p) for p in perm) == list(range(n)), "perm is not a permutation"
    if words == 1 and n >= 600:
        # fp64 at n >= 600: the mpmath residual takes ~5 s, so np.longdouble (64-bit significand)
        # computes it: its own error, n 2^-64 |L||U||v|, is 2^-14 of the bound
        ld = np.longdouble
        Lm = np.tril(LUl[0], -1).astype(ld) + np.eye(n, dtype=ld)
        Um = np.triu(LUl[0]).astype(ld)
        Lf, Uf = np.abs(Lm).astype(float), np.abs(Um).astype(float)
        worst = 0.0
        for which in (None, 0, 1):
            v = np.ones(n, dtype=np.int64) if which is None else sketch_weights(n, which)
            r = np.abs(A[perm, :].astype(ld) @ v.astype(ld) - Lm @ (Um @ v.astype(ld))).astype(float)
            bound = 8.0 * n * EPS[1] * (Lf @ (Uf @ np.abs(v).astype(float)))
            worst = max(worst, float(np.max(r / bound)))
        return worst
    with mpmath.workprec(PREC):
        Am = A if A.dtype == object else _mpf(A)
        LU = _exact(LUl)
        Lf = np.tril(np.abs(LUl[0]), -1) + np.eye(n)
        Uf = np.triu(np.abs(LUl[0]))
        worst = 0.0
        for which in (None, 0, 1):
            v = np.ones(n, dtype=np.int64) if which is None else sketch_weights(n, which)
            vm = [mpmath.mpf(int(x)) for x in v]
            Uv = [mpmath.fdot(LU[i, i:], vm[i:]) for i in range(n)]
            LUv = [Uv[i] + mpmath.fdot(LU[i, :i], Uv[:i]) for i in range(n)]
            Av = [mpmath.fdot(Am[int(perm[i]), :], vm) for i in range(n)]
            r = np.array([float(abs(a - b)) for a, b in zip(Av, LUv)])
            bound = 8.0 * n * EPS[words] * (Lf @ (Uf @ np.abs(v).astype(float)))
            assert np.all(bound > 0)
            worst = max(worst, float(np.max(r / bound)))
    return worst


def _factor(pk, terms_list, words):
    LU, perms, info = pk.getrf([_block(t) for t in terms_list], precision_words=words, raw_limbs=True)
    return LU, perms, info


# just past each old bound and ragged against the 16-wide panel, and the one-CU kernel at its
# largest size (the comparison figure of the bound)
SIZES = [(4, 157), (4, 161), (2, 313), (2, 321), (1, 625), (1, 641), (4, 156), (2, 312), (1, 624)]


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["random", "graded", "antidiag"])
@pytest.mark.parametrize("words,n", SIZES, ids=[f"w{w}-n{n}" for w, n in SIZES])
def test_getrf_probing_residual(pk, words, n, kind):
    terms = _matrix(pk, n, words, kind)
    LU, perms, info = _factor(pk, [terms], words)
    assert info.tolist() == [0]
    ratio = probe_ratio(_block(terms), LU[0], perms[0], words)
    print(f"getrf words={words} n={n} kind={kind} ({'chain' if n > BOUND[words] else 'one-CU'}): "
          f"residual / bound = {ratio:.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("words,sizes", [(4, [161, 33, 1, 16, 17]), (2, [321, 33, 1, 16, 17]),
                                         (1, [641, 33, 1, 16, 17])], ids=["qd", "dd", "fp64"])
def test_getrf_mixed_batch(pk, words, sizes):
    """One batch of mixed sizes (the first past the bound, so the whole batch takes the chain):
    blocks smaller than the current panel leave the chain early."""
    tl = [_matrix(pk, n, words, b % 3, seed=23 + b) for b, n in enumerate(sizes)]
    LU, perms, info = _factor(pk, tl, words)
    assert info.tolist() == [0] * len(sizes)
    for b, n in enumerate(sizes):
        ratio = probe_ratio(_block(tl[b]), LU[b], perms[b], words)
        print(f"mixed batch words={words} n={n}: residual / bound = {ratio:.3e}")
        assert ratio <= 1.0
    # the same blocks one by one give the same factors (a block's result does not depend on
    # its neighbours in the batch)
    for b in (1, 4):
        LU1, p1, i1 = _factor(pk, [tl[0], tl[b]], words)
        assert np.array_equal(p1[1], perms[b]) and np.array_equal(LU1[1], LU[b])


@pytest.mark.parametrize("kind", [0, 2], ids=["random", "antidiag"])
@pytest.mark.parametrize("words,n", [(2, 16), (2, 17), (2, 100), (2, 312), (4, 16), (4, 17), (4, 100),
                                     (4, 156)], ids=lambda x: str(x))
def test_chain_is_bitwise_the_one_cu_kernel(pk, monkeypatch, words, n, kind):
    """Double-double and quad-double: the chain (CLRSDP_LU_BLK=1) against getrf_batched (unset) on
    the same matrix: identical perm and every limb of L and U equal.  The same with the chain's
    panel kept in global memory (CLRSDP_LU_PANEL_LDS=0: the path of panels beyond LDS)."""
    terms = _matrix(pk, n, words, kind, seed=31)
    monkeypatch.delenv("CLRSDP_LU_BLK", raising=False)
    LU0, p0, i0 = _factor(pk, [terms], words)
    monkeypatch.setenv("CLRSDP_LU_BLK", "1")
    LU1, p1, i1 = _factor(pk, [terms], words)
    monkeypatch.setenv("CLRSDP_LU_PANEL_LDS", "0")
    LU2, p2, i2 = _factor(pk, [terms], words)
    assert i0.tolist() == i1.tolist() == i2.tolist() == [0]
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[0], p2[0])
    assert LU0[0].shape == (words, n, n)
    assert np.array_equal(LU0[0], LU1[0]), int(np.sum(LU0[0] != LU1[0]))
    assert np.array_equal(LU0[0], LU2[0]), int(np.sum(LU0[0] != LU2[0]))


@pytest.mark.parametrize("n", [16, 17, 100, 624])
def test_chain_against_one_cu_fp64(pk, monkeypatch, n):
    """fp64: identical perm and the probing bound for both kernels (whether the values are also
    bitwise equal is up to the compiler's contractions, and is printed)."""
    terms = _matrix(pk, n, 1, 0, seed=31)
    monkeypatch.delenv("CLRSDP_LU_BLK", raising=False)
    LU0, p0, i0 = _factor(pk, [terms], 1)
    monkeypatch.setenv("CLRSDP_LU_BLK", "1")
    LU1, p1, i1 = _factor(pk, [terms], 1)
    assert i0.tolist() == i1.tolist() == [0]
    assert np.array_equal(p0[0], p1[0])
    r0 = probe_ratio(terms[0], LU0[0], p0[0], 1)
    r1 = probe_ratio(terms[0], LU1[0], p1[0], 1)
    print(f"fp64 n={n}: residual / bound one-CU {r0:.3e}, chain {r1:.3e}; "
          f"limbs equal: {np.array_equal(LU0[0], LU1[0])}")
    assert r0 <= 1.0 and r1 <= 1.0


def test_lu_blk_0_keeps_the_old_bound(pk, monkeypatch):
    from clrsdp_amd import _lib as L
    monkeypatch.setenv("CLRSDP_LU_BLK", "0")
    with pytest.raises(L.ClrsdpError) as ei:
        pk.getrf([np.eye(157)], precision_words=4)
    assert ei.value.code == L.E_ARG
    LU, perms, info = pk.getrf([np.eye(156)], precision_words=4, raw_limbs=True)
    assert info.tolist() == [0] and np.array_equal(LU[0][0], np.eye(156))


def test_panel_beyond_lds(pk):
    """Quad-double n = 321: the first panels (more than 304 rows of 16 quad-doubles) do not fit
    in LDS and are factored in place in global memory."""
    terms = _matrix(pk, 321, 4, 2, seed=41)
    LU, perms, info = _factor(pk, [terms], 4)
    assert info.tolist() == [0]
    ratio = probe_ratio(_block(terms), LU[0], perms[0], 4)
    print(f"getrf words=4 n=321 (global panel): residual / bound = {ratio:.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("words,big", [(4, 157), (2, 313), (1, 625)], ids=["qd", "dd", "fp64"])
@pytest.mark.parametrize("cols", [(37,), (37, 90)], ids=["col37", "col37+90"])
def test_zero_pivot_is_the_first_failing_column(pk, words, big, cols):
    """A batch of three whose middle matrix has column 37 exactly zero: info = [0, 38, 0] (also
    with column 90 zero as well: the first failure stays), the outer two are factored."""
    sizes = [big, 100, 50]
    tl = [_matrix(pk, n, words, 0, seed=51 + b) for b, n in enumerate(sizes)]
    for t in tl[1]:
        for c in cols:
            t[:, c] = 0.0
    LU, perms, info = _factor(pk, tl, words)
    assert info.tolist() == [0, 38, 0]
    assert sorted(perms[1].tolist()) == list(range(100))
    for b in (0, 2):
        ratio = probe_ratio(_block(tl[b]), LU[b], perms[b], words)
        print(f"zero-pivot batch words={words} n={sizes[b]}: residual / bound = {ratio:.3e}")
        assert ratio <= 1.0
