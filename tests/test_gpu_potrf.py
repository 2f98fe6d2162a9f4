"""GPU tests of the stand-alone Cholesky (clrsdp_potrf / solver.potrf, include/clrsdp.h): every
kernel behind MatPlan::potrf (the factor L) and CholInvPlan::launch (L^-1) on both sides of every
size boundary of its dispatch, against mpmath at 320 bits and a-priori
bounds.  Inputs: potrf_cases (kinds 0-3), handed over as limbs, so the exact A is the limb sum.

eps = 2^-53 / 2^-104 / 2^-206; the margin 8 is the one of the getrf and trsm tests.

Factor form.  For v in {ones, two +-1 sketches}: r = A v - L (L^T v), from tril of the device
result, against the backward-error bound of the Cholesky recurrence (Higham, Accuracy and
Stability, Thm 10.3: |A - L L^T| <= gamma_{n+1} |L| |L|^T):
    |r_i| <= 8 n eps (|L| (|L|^T |v|))_i .
The potrf_blk_* chain alone forms its panel as A_ik (L_kk^-1)^T with an explicit inverse of the
16 x 16 diagonal block, whose backward error carries |L_kk^-1| |L_kk| (as
test_stage_parity_dd_late_iterate documents): its bound is multiplied by
c = max_k || |L_kk^-1| |L_kk| ||_inf over the diagonal blocks, from the leading limbs of the
device's L.  On kinds 0-2 c is small (asserted <= 64) and the plain bound has to hold as well.

Inverse form.  E = X A X^T - I over the full matrix (mpmath at multi-word, np.longdouble at
fp64), M = |X| |X^-1| with X^-1 from a triangular solve in the same precision:
    |E_ij| <= 3 * 8 n eps (M M^T)_ij .
Derivation: the computed factor has A + dA = L L^T, |dA| <= g |L| |L|^T, and the computed inverse
X L = I + R, |R| <= g |X| |L| (g = gamma_n).  Then X A X^T = (I + R)(I + R)^T - X dA X^T
= I + R + R^T - X dA X^T + O(g^2), and with |L| = |X^-1| to first order |X dA X^T| <= g M M^T,
|R| <= g M <= g M M^T and |R^T| <= g M M^T (M_jj >= |X_jj| |X^-1_jj| = 1, so (M M^T)_ij >=
M_ij M_jj >= M_ij and >= M_ii M_ji): three terms of g M M^T each.  triu(X, 1) is exactly zero,
written by the kernel (the entry point fills the buffer with NaN bytes before the launch).

Every test prints the kernel, n and the largest ratio to its bound.
"""
import functools
import re

import mpmath
import numpy as np
import pytest

import potrf_cases as pc
from helpers import sketch_weights

pytestmark = pytest.mark.gpu

EPS = pc.EPS
PREC = pc.PREC
KINDS = {0: "spd", 1: "graded", 2: "known", 3: "illcond"}
WNAME = {1: "fp64", 2: "dd", 4: "qd"}
_mpf = np.frompyfunc(mpmath.mpf, 1, 1)
_flt = np.frompyfunc(float, 1, 1)

# (kernel, words, CLRSDP_POTRF_BLK=0, sizes): the dispatch of MatPlan::potrf
FACTOR = [
    ("potrf_batched<double,16,256>", 1, False, [1, 2, 15, 16, 17, 33, 129, 257]),
    ("chol_lookahead<dd,64>", 2, False, [1, 2, 17, 63, 64]),
    ("potrf_blk<dd,16>", 2, False, [65, 79, 80, 81, 128, 129, 160]),
    ("chol_lookahead<dd,128>", 2, True, [65, 127, 128]),
    ("potrf_batched<dd,16,1024>", 2, True, [129, 160]),
    ("chol_lookahead<qd,LDL,64>", 4, False, [1, 2, 17, 63, 64]),
    ("potrf_batched<qd,16,256>", 4, False, [65, 80, 100]),
]
# (kernel, words, sizes): the dispatch of CholInvPlan::launch
INVERSE = [
    ("chol_inv_tiles<32>", 1, [1, 2, 8, 9, 16, 17, 31, 32]),
    ("chol_inv_tiles<64>", 1, [33, 63, 64]),
    ("chol_inv_tiles<128>", 1, [65, 100, 128]),
    ("chol_inv_tiles<256>", 1, [129, 200, 256]),
    ("chol_lookahead<dd,inv,32>", 2, [1, 2, 8, 9, 18, 31, 32]),
    ("chol_lookahead<dd,inv,64>", 2, [33, 40, 63, 64]),
    ("chol_lookahead<qd,inv,LDL,32>", 4, [1, 2, 8, 9, 18, 31, 32]),
    ("chol_lookahead<qd,inv,LDL,64>", 4, [33, 40, 63, 64]),
]
FACTOR_CASES = [(k, w, b0, n) for k, w, b0, sizes in FACTOR for n in sizes]
INVERSE_CASES = [(k, w, n) for k, w, sizes in INVERSE for n in sizes]
_fid = lambda c: f"{c[0]}-n{c[3]}"  # noqa: E731
_iid = lambda c: f"{c[0]}-n{c[2]}"  # noqa: E731
# one row per kernel: (kernel, words, blk0, inverse, largest size, a size for the single-size cases)
ONE = {"potrf_batched<double,16,256>": 129, "chol_lookahead<dd,64>": 64, "potrf_blk<dd,16>": 81,
       "chol_lookahead<dd,128>": 127, "potrf_batched<dd,16,1024>": 129,
       "chol_lookahead<qd,LDL,64>": 63, "potrf_batched<qd,16,256>": 80,
       "chol_inv_tiles<32>": 32, "chol_inv_tiles<64>": 63, "chol_inv_tiles<128>": 100,
       "chol_inv_tiles<256>": 200, "chol_lookahead<dd,inv,32>": 31, "chol_lookahead<dd,inv,64>": 40,
       "chol_lookahead<qd,inv,LDL,32>": 31, "chol_lookahead<qd,inv,LDL,64>": 40}
KERNELS = [(k, w, b0, False, max(s), ONE[k]) for k, w, b0, s in FACTOR] + \
          [(k, w, False, True, max(s), ONE[k]) for k, w, s in INVERSE]
_kid = lambda c: c[0]  # noqa: E731


@functools.lru_cache(maxsize=None)
def _limbs(n, words, kind, seed=11):
    """the input block as (words, n, n) limbs: computed once per case, never modified"""
    from clrsdp_amd import instance as inst
    a = pc.spd_limbs(inst, n, words, kind, seed)
    a.setflags(write=False)
    return a


def _blk_env(monkeypatch, blk0):
    if blk0:
        monkeypatch.setenv("CLRSDP_POTRF_BLK", "0")
    else:
        monkeypatch.delenv("CLRSDP_POTRF_BLK", raising=False)


def _run(pk, blocks, words, inverse):
    out, info = pk.potrf(blocks, inverse=inverse, precision_words=words, raw_limbs=True)
    return out, info.tolist()


def _tril(limbs):
    return np.tril(limbs)        # (the last two axes)


def chain_c(L0):
    """max_k || |L_kk^-1| |L_kk| ||_inf over the 16 x 16 diagonal blocks of the leading limb"""
    n = L0.shape[0]
    c = 1.0
    for k0 in range(0, n, 16):
        D = np.tril(L0[k0:k0 + 16, k0:k0 + 16])
        c = max(c, float(np.max(np.sum(np.abs(np.linalg.inv(D)) @ np.abs(D), axis=1))))
    return c


def factor_ratio(A_limbs, L_limbs, words):
    """max_i |r_i| / (8 n eps (|L| (|L|^T |v|))_i) over the three probing vectors; only tril of
    the device result is used"""
    n = A_limbs.shape[1]
    Ll = _tril(L_limbs)
    assert np.all(np.isfinite(Ll)), "L is not finite"
    Lf = np.abs(Ll[0])
    vs = [np.ones(n, dtype=np.int64), sketch_weights(n, 0), sketch_weights(n, 1)]
    worst = 0.0
    if words == 1 and n >= 250:
        # np.longdouble (64-bit significand): its own error, n 2^-64 |L| |L|^T |v|, is 2^-14 of
        # the bound
        ld = np.longdouble
        Lm, Am = Ll[0].astype(ld), A_limbs[0].astype(ld)
        for v in vs:
            r = np.abs(Am @ v.astype(ld) - Lm @ (Lm.T @ v.astype(ld))).astype(float)
            bound = 8.0 * n * EPS[1] * (Lf @ (Lf.T @ np.abs(v).astype(float)))
            worst = max(worst, float(np.max(r / bound)))
        return worst
    with mpmath.workprec(PREC):
        Am, Lm = _mpf(pc.exact(A_limbs)), _mpf(pc.exact(Ll))
        for v in vs:
            vm = [mpmath.mpf(int(x)) for x in v]
            Ltv = [mpmath.fdot(Lm[i:, i], vm[i:]) for i in range(n)]
            LLv = [mpmath.fdot(Lm[i, :i + 1], Ltv[:i + 1]) for i in range(n)]
            Av = [mpmath.fdot(Am[i, :], vm) for i in range(n)]
            r = np.array([float(abs(a - b)) for a, b in zip(Av, LLv)])
            bound = 8.0 * n * EPS[words] * (Lf @ (Lf.T @ np.abs(v).astype(float)))
            assert np.all(bound > 0)
            worst = max(worst, float(np.max(r / bound)))
    return worst


def inverse_ratio(A_limbs, X_limbs, words):
    """max_ij |E_ij| / (3 * 8 n eps (M M^T)_ij), E = X A X^T - I, M = |X| |X^-1|; also asserts
    that the strict upper triangle of X is exactly zero in every limb"""
    n = A_limbs.shape[1]
    assert np.all(np.isfinite(X_limbs)), "L^-1 is not finite (an entry the kernel did not write is NaN)"
    assert not np.triu(X_limbs, 1).any(), "L^-1 is not exactly zero above the diagonal"
    if words == 1:
        ld = np.longdouble
        X, A = X_limbs[0].astype(ld), A_limbs[0].astype(ld)
        A = np.tril(A) + np.tril(A, -1).T
        E = np.abs(X @ A @ X.T - np.eye(n, dtype=ld)).astype(float)
        Y = np.zeros((n, n), dtype=ld)               # X^-1 by forward substitution, row by row
        for i in range(n):
            e = np.zeros(n, dtype=ld)
            e[i] = 1
            Y[i] = (e - X[i, :i] @ Y[:i]) / X[i, i]
        M = (np.abs(X) @ np.abs(Y)).astype(float)
    else:
        with mpmath.workprec(PREC):
            X, A = _mpf(pc.exact(X_limbs)), _mpf(pc.exact(A_limbs))
            XA = np.array([[mpmath.fdot(X[i, :i + 1], A[:i + 1, j]) for j in range(n)] for i in range(n)],
                          dtype=object).reshape(n, n)
            E = np.array([[float(abs(mpmath.fdot(XA[i, :j + 1], X[j, :j + 1]) - (1 if i == j else 0)))
                           for j in range(n)] for i in range(n)]).reshape(n, n)
            Y = np.empty((n, n), dtype=object)
            Y[:] = mpmath.mpf(0)
            for i in range(n):
                for j in range(i + 1):
                    s = (1 if i == j else 0) - mpmath.fdot(X[i, j:i], Y[j:i, j])
                    Y[i, j] = s / X[i, i]
            Xa = np.abs(X_limbs[0])
            Ya = np.abs(_flt(Y).astype(float)).reshape(n, n)
            M = Xa @ Ya
    bound = 3.0 * 8.0 * n * EPS[words] * (M @ M.T)
    assert np.all(bound > 0)
    return float(np.max(E / bound))


def _check_factor(kernel, A, L, words, kind, what=""):
    """the probing bound of the module docstring on one block; returns (ratio, c)"""
    n = A.shape[1]
    ratio = factor_ratio(A, L, words)
    chain = kernel.startswith("potrf_blk")
    c = chain_c(np.tril(L[0])) if chain else 1.0
    print(f"{kernel} {what}n={n} kind={KINDS[kind]}: residual / bound = {ratio:.3e}"
          + (f", c = {c:.2f}, residual / (c bound) = {ratio / c:.3e}" if chain else ""))
    if chain and kind != 3:
        assert c <= 64.0, c          # the allowance cannot hide anything on these kinds
        assert ratio <= 1.0
    assert ratio <= c
    return ratio, c


def _check_inverse(kernel, A, X, words, kind, what=""):
    ratio = inverse_ratio(A, X, words)
    print(f"{kernel} {what}n={A.shape[1]} kind={KINDS[kind]}: |X A X^T - I| / bound = {ratio:.3e}")
    assert ratio <= 1.0
    return ratio


def _check(kernel, inverse, A, R, words, kind, what=""):
    return _check_inverse(kernel, A, R, words, kind, what) if inverse else \
        _check_factor(kernel, A, R, words, kind, what)


# ---------------------------------------------------------------- every size of every kernel

@pytest.mark.parametrize("kind", [0, 1, 3], ids=[KINDS[k] for k in (0, 1, 3)])
@pytest.mark.parametrize("case", FACTOR_CASES, ids=_fid)
def test_potrf_probing_residual(pk, monkeypatch, case, kind):
    """info = 0 and the probing bound, for kinds 0, 1 and 3 (kind 3 at double-double and
    quad-double: the word's full width is kept, test_potrf_host.py)."""
    kernel, words, blk0, n = case
    _blk_env(monkeypatch, blk0)
    A = _limbs(n, words, kind)
    (L,), info = _run(pk, [A], words, False)
    assert info == [0]
    _check_factor(kernel, A, L, words, kind)


@pytest.mark.parametrize("kind", [0, 1, 3], ids=[KINDS[k] for k in (0, 1, 3)])
@pytest.mark.parametrize("case", INVERSE_CASES, ids=_iid)
def test_potrf_inverse_residual(pk, case, kind):
    kernel, words, n = case
    A = _limbs(n, words, kind)
    (X,), info = _run(pk, [A], words, True)
    assert info == [0]
    _check_inverse(kernel, A, X, words, kind)


@pytest.mark.parametrize("case", KERNELS, ids=_kid)
def test_potrf_known_factor(pk, monkeypatch, case):
    """Kind 2, L = D tril(ones) and L^-1 = (I - subdiagonal) D^-1 exactly: the bound of the form,
    every entry within 8 n eps relative of the known value, and the exact zeros of the known L^-1
    (below its subdiagonal) below 8 n eps in absolute value, although the entries beside them
    reach 2^39."""
    kernel, words, blk0, inverse, _, n = case
    _blk_env(monkeypatch, blk0)
    A = _limbs(n, words, 2)
    (R,), info = _run(pk, [A], words, inverse)
    assert info == [0]
    _check(kernel, inverse, A, R, words, 2)
    K = pc.known_factor(n, inverse)
    Rl = _tril(R)
    exact_bits = np.array_equal(Rl[0], K) and not Rl[1:].any()
    print(f"{kernel} n={n} known factor: bitwise exact: {exact_bits}")
    tol = 8.0 * n * EPS[words]
    with mpmath.workprec(PREC):
        err = np.abs(_flt(_mpf(pc.exact(Rl)) - _mpf(K)).astype(float))
    nz = K != 0
    assert np.all(err[nz] <= tol * np.abs(K[nz])), float(np.max(err[nz] / np.abs(K[nz])))
    zero = ~nz & np.tril(np.ones((n, n), dtype=bool))
    assert np.all(err[zero] <= tol), float(np.max(err[zero], initial=0.0))


# ---------------------------------------------------------------- one test per property

def _mixed_sizes(nmax):
    return [nmax] + [min(s, nmax) for s in (1, 16, 17, 33)]


@pytest.mark.parametrize("case", KERNELS, ids=_kid)
def test_potrf_mixed_batch(pk, monkeypatch, case):
    """One batch [nmax, 1, 16, 17, 33] (clipped to the kernel's range; nmax chooses the kernel,
    so the small blocks ride in a launch sized by the large one): every block meets its bound,
    and blocks 1 and 4 are bitwise the same block's result in a batch [nmax block, that block]."""
    kernel, words, blk0, inverse, nmax, _ = case
    _blk_env(monkeypatch, blk0)
    sizes = _mixed_sizes(nmax)
    kinds = [0, 1, 2, 3, 0]
    As = [_limbs(n, words, kinds[b], seed=23 + b) for b, n in enumerate(sizes)]
    R, info = _run(pk, As, words, inverse)
    assert info == [0] * len(sizes)
    for b in range(len(sizes)):
        _check(kernel, inverse, As[b], R[b], words, kinds[b], what=f"mixed block {b} ")
    for b in (1, 4):
        R1, i1 = _run(pk, [As[0], As[b]], words, inverse)
        assert i1 == [0, 0]
        assert np.array_equal(_tril(R1[1]), _tril(R[b]))
        assert np.array_equal(_tril(R1[0]), _tril(R[0]))


@pytest.mark.parametrize("case", KERNELS, ids=_kid)
def test_potrf_reads_the_lower_triangle_only(pk, monkeypatch, case):
    """NaN in every limb of the strict upper triangle of the input (STAGE_SCHUR may assemble the
    lower triangle of S alone): the result's lower triangle is bitwise the symmetric input's."""
    kernel, words, blk0, inverse, nmax, _ = case
    _blk_env(monkeypatch, blk0)
    A = _limbs(nmax, words, 0)
    An = A.copy()
    An[:, np.triu(np.ones((nmax, nmax), dtype=bool), 1)] = np.nan
    (R,), info = _run(pk, [A], words, inverse)
    (Rn,), infon = _run(pk, [An], words, inverse)
    assert info == [0] and infon == [0]
    assert np.all(np.isfinite(_tril(Rn)))
    assert np.array_equal(_tril(Rn), _tril(R))
    if inverse:
        assert not np.triu(Rn, 1).any()


@pytest.mark.parametrize("e", [400, -400], ids=["up", "down"])
@pytest.mark.parametrize("case", KERNELS, ids=_kid)
def test_potrf_scale(pk, monkeypatch, case, e):
    """Kind 0 with every limb multiplied by 2^e, e = +-400 (exact): info = 0 and the result is
    the unscaled one times 2^(e/2) (L) or 2^(-e/2) (L^-1), bitwise; where it is not bitwise
    (printed), its bound must hold at that scale."""
    kernel, words, blk0, inverse, _, n = case
    _blk_env(monkeypatch, blk0)
    A = _limbs(n, words, 0)
    As = np.ldexp(A, e)
    (R,), info = _run(pk, [A], words, inverse)
    (Rs,), infos = _run(pk, [As], words, inverse)
    assert info == [0] and infos == [0]
    assert np.all(np.isfinite(_tril(Rs)))
    same = np.array_equal(_tril(Rs), np.ldexp(_tril(R), -e // 2 if inverse else e // 2))
    print(f"{kernel} n={n} scale 2^{e}: bitwise the unscaled result: {same}")
    if not same:
        _check(kernel, inverse, As, Rs, words, 0, what=f"scale 2^{e} ")


@pytest.mark.parametrize("case", KERNELS, ids=_kid)
def test_potrf_failure_column(pk, monkeypatch, case):
    """A[k, k] lowered by 2 l_kk^2 (l_kk from a float Cholesky): pivot k turns negative while
    the leading k x k minor is untouched.  In a batch [good, bad, good], k in {0, 5, 16, n - 1}:
    info = [0, k + 1, 0] -- chol_inv_tiles reports the first column of the 16-column diagonal
    tile that holds the pivot, 16 (k // 16) + 1 -- and the same with NaN at A[k, k].  The good
    blocks are complete (the same bits in every batch) and meet their bounds."""
    kernel, words, blk0, inverse, _, n = case
    _blk_env(monkeypatch, blk0)
    good0, good2, A = _limbs(n, words, 0, seed=51), _limbs(max(n // 2, 1), words, 1, seed=52), _limbs(n, words, 0, seed=53)
    lkk = np.diag(np.linalg.cholesky(A[0]))
    first = None
    for k in (0, 5, 16, n - 1):
        for nan in (False, True):
            bad = A.copy()
            if nan:
                bad[:, k, k] = np.nan
            else:
                bad[0, k, k] -= 2.0 * lkk[k] ** 2
            R, info = _run(pk, [good0, bad, good2], words, inverse)
            want = 16 * (k // 16) + 1 if kernel.startswith("chol_inv_tiles") else k + 1
            print(f"{kernel} n={n} k={k} {'NaN' if nan else 'negative'} pivot: info = {info}")
            assert info == [0, want, 0]
            if first is None:
                first = R
                _check(kernel, inverse, good0, R[0], words, 0, what="beside a failed block: ")
                _check(kernel, inverse, good2, R[2], words, 1, what="beside a failed block: ")
            else:
                assert np.array_equal(_tril(R[0]), _tril(first[0]))
                assert np.array_equal(_tril(R[2]), _tril(first[2]))


# ---------------------------------------------------------------- potrf_batched's size bound

def _limit(pk, words):
    """potrf_batched's largest n at this word type, read back from the refusal's message"""
    from clrsdp_amd import _lib as L
    with pytest.raises(L.ClrsdpError) as ei:
        pk.potrf([np.eye(1500)], precision_words=words)
    assert ei.value.code == L.E_ARG
    assert "potrf_batched" in str(ei.value)
    return int(re.search(r"n <= (\d+)", str(ei.value)).group(1))


@pytest.mark.parametrize("words,blk0", [(4, False), (1, False), (2, True)], ids=["qd", "fp64", "dd-blk0"])
def test_potrf_batched_size_bound(pk, monkeypatch, words, blk0):
    """Past the n at which potrf_batched's 16-column panel and its static LDS fit one CU the call
    is CLRSDP_E_ARG (no launch is made: the runtime's refusal of one would be CLRSDP_E_HIP); at
    the limit the identity factors to the identity."""
    from clrsdp_amd import _lib as L
    _blk_env(monkeypatch, blk0)
    lim = _limit(pk, words)
    print(f"potrf_batched {WNAME[words]}: n <= {lim}")
    sz = {1: 8, 2: 16, 4: 32}[words]
    assert sz * (256 + 16 * lim) <= 160 * 1024 < sz * (256 + 16 * (lim + 1)) + 16 * sz + 16
    with pytest.raises(L.ClrsdpError) as ei:
        pk.potrf([np.eye(lim + 1)], precision_words=words)
    assert ei.value.code == L.E_ARG
    (R,), info = _run(pk, [np.eye(lim)], words, False)
    assert info == [0]
    assert np.array_equal(np.tril(R[0]), np.eye(lim)) and not R[1:].any()


def test_double_double_chain_has_no_size_bound(pk, monkeypatch):
    """the default double-double path past 64 (potrf_blk_*) is not potrf_batched: no refusal"""
    monkeypatch.delenv("CLRSDP_POTRF_BLK", raising=False)
    (R,), info = _run(pk, [np.eye(700)], 2, False)
    assert info == [0] and np.array_equal(np.tril(R[0]), np.eye(700)) and not R[1:].any()


def test_solver_past_the_bound_is_e_arg_at_the_cholesky(pk):
    """Quad-double dim_S = 320 (the shape of test_gpu_lu_large.py with N = 320): S_j would be
    factored by potrf_batched past its bound.  The handle itself is created -- handles past the
    bound run the stages before FACTOR (test_schur_stage_beyond_64_row_blocks: fp64 dim_S up to
    4097) and FACTOR by pivoted LU, which has no bound -- and the Cholesky FACTOR is refused with
    CLRSDP_E_ARG before its launch, in the stage-by-stage run and in the (captured) loop body."""
    from clrsdp_amd import _lib as L
    cons, b = pk.synth(seed=3, J=2, L=1, rank=1, n_y=8, delta=32, N=320)
    bi = pk.get_block_info(cons)
    P = pk.make_params("0.3", "0.1", "0.7", 0)
    dev = pk.DeviceSolver(cons, b, bi, precision_words=4)
    try:
        dev.set_factorization(0)
        dev.set_state(*pk.initial_point(bi, 10.0, 10.0))
        for s in (L.STAGE_MU_R, L.STAGE_XINV, L.STAGE_SCHUR):
            dev.run_stage(s, P, False)
        with pytest.raises(L.ClrsdpError) as ei:
            dev.run_stage(L.STAGE_FACTOR, P, False)
        assert ei.value.code == L.E_ARG and "potrf_batched" in str(ei.value)
        dev.set_factorization(L.FACT_LU_SQ)
        dev.run_stage(L.STAGE_FACTOR, P, False)       # (LU: no size bound)
        dev.set_factorization(0)
        with pytest.raises(L.ClrsdpError) as ei:
            dev.iterate(P, False)
        assert ei.value.code == L.E_ARG and "potrf_batched" in str(ei.value)
    finally:
        dev.close()
