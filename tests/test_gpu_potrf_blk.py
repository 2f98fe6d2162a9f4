"""GPU tests of the blocked Cholesky chains across workgroups at fp64 (potrf64_*, NB = 16-column
panels, the trailing update on the fp64 matrix cores) and quad-double (potrf_blk_* in the LDL
form, 16-column panels), which CLRSDP_POTRF_BLK=1 puts in the place of potrf_batched
(MatPlan::potrf).  Every case sets the switch with monkeypatch.

Inputs, eps, the margin 8, PREC and the probing-residual check are those of test_gpu_potrf.py:
    |A v - L (L^T v)|_i <= 8 n eps (|L| (|L|^T |v|))_i   for v = ones and the two +-1 sketches.
The fp64 chain forms its panel by forward substitution against L_kk, so its bound is the plain
one (c = 1).  The quad-double chain forms it as a product with an explicit L_kk^-1 of the
16 x 16 diagonal block and gets the allowance of the double-double chain there,
c = max_k || |L_kk^-1| |L_kk| ||_inf: c <= 64 and the plain bound as well on kinds 0-2
(test_gpu_potrf._check_factor, keyed on the kernel's name).
"""
import mpmath
import numpy as np
import pytest

import potrf_cases as pc
import test_gpu_lu_large as lul
import test_gpu_potrf as tp

pytestmark = pytest.mark.gpu

NB = 16                                   # MatPlan::BLK64_NB
K64, KQD = f"potrf64<{NB}>", "potrf_blk<qd,LDL,16>"
SIZES = {1: sorted({1, 2, 15, 16, 17, NB - 1, NB, NB + 1, 2 * NB + 1, 129, 257}), 4: [65, 79, 80, 81, 100]}
KERNEL = {1: K64, 4: KQD}
CASES = [(w, n) for w in (1, 4) for n in SIZES[w]]
_cid = lambda c: f"{tp.WNAME[c[0]]}-n{c[1]}"  # noqa: E731
WORDS = pytest.mark.parametrize("words", [1, 4], ids=["fp64", "qd"])


@pytest.fixture(autouse=True)
def _chain_on(monkeypatch):
    monkeypatch.setenv("CLRSDP_POTRF_BLK", "1")


@pytest.mark.parametrize("kind", [0, 1, 3], ids=[tp.KINDS[k] for k in (0, 1, 3)])
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_chain_probing_residual(pk, case, kind):
    words, n = case
    A = tp._limbs(n, words, kind)
    (L,), info = tp._run(pk, [A], words, False)
    assert info == [0]
    tp._check_factor(KERNEL[words], A, L, words, kind)
    assert not np.triu(L, 1).any(), "L is not exactly zero above the diagonal"


@pytest.mark.parametrize("words,n", [(1, 129), (4, 81)], ids=["fp64-129", "qd-81"])
def test_chain_known_factor(pk, words, n):
    """Kind 2: every entry within 8 n eps of L = D tril(ones)."""
    A = tp._limbs(n, words, 2)
    (R,), info = tp._run(pk, [A], words, False)
    assert info == [0]
    tp._check_factor(KERNEL[words], A, R, words, 2)
    K = pc.known_factor(n, False)
    Rl = np.tril(R)
    tol = 8.0 * n * pc.EPS[words]
    with mpmath.workprec(pc.PREC):
        err = np.abs(tp._flt(tp._mpf(pc.exact(Rl)) - tp._mpf(K)).astype(float))
    nz = K != 0
    print(f"{KERNEL[words]} n={n} known factor: max relative error / (8 n eps) = "
          f"{float(np.max(err[nz] / np.abs(K[nz]))) / tol:.3e}")
    assert np.all(err[nz] <= tol * np.abs(K[nz]))
    assert not np.triu(R, 1).any()


@pytest.mark.parametrize("words,sizes", [(1, [257, 1, 16, 17, 33]), (4, [100, 65, 80])], ids=["fp64", "qd"])
def test_chain_mixed_batch(pk, words, sizes):
    """Every block of one batch meets its bound (the small ones leave the launches of the panels
    past their size), and a small block's lower triangle is bitwise the same in a batch of two."""
    kinds = [0, 1, 2, 3, 0]
    As = [tp._limbs(n, words, kinds[b], seed=23 + b) for b, n in enumerate(sizes)]
    R, info = tp._run(pk, As, words, False)
    assert info == [0] * len(sizes)
    for b in range(len(sizes)):
        tp._check_factor(KERNEL[words], As[b], R[b], words, kinds[b], what=f"mixed block {b} ")
    for b in (1, len(sizes) - 1):
        R1, i1 = tp._run(pk, [As[0], As[b]], words, False)
        assert i1 == [0, 0]
        assert np.array_equal(np.tril(R1[1]), np.tril(R[b]))
        assert np.array_equal(np.tril(R1[0]), np.tril(R[0]))


@pytest.mark.parametrize("words,n", [(1, 257), (4, 100)], ids=["fp64-257", "qd-100"])
def test_chain_reads_the_lower_triangle_only(pk, words, n):
    A = tp._limbs(n, words, 0)
    An = A.copy()
    An[:, np.triu(np.ones((n, n), dtype=bool), 1)] = np.nan
    (R,), info = tp._run(pk, [A], words, False)
    (Rn,), infon = tp._run(pk, [An], words, False)
    assert info == [0] and infon == [0]
    assert np.all(np.isfinite(np.tril(Rn)))
    assert np.array_equal(np.tril(Rn), np.tril(R))
    assert not np.triu(Rn, 1).any()


@pytest.mark.parametrize("words,n", [(1, 129), (4, 81)], ids=["fp64-129", "qd-81"])
def test_chain_failure_column(pk, words, n):
    """Batch [good, bad, good], pivot k of the bad block once negative (A[k, k] lowered by
    2 l_kk^2) and once NaN, k in {0, 5, 16, NB, n - 1}: info = [0, k + 1, 0], the good blocks the
    same bits in every batch and within their bounds."""
    good0, good2, A = tp._limbs(n, words, 0, seed=51), tp._limbs(n // 2, words, 1, seed=52), tp._limbs(n, words, 0, seed=53)
    lkk = np.diag(np.linalg.cholesky(A[0]))
    first = None
    for k in sorted({0, 5, 16, NB, n - 1}):
        for nan in (False, True):
            bad = A.copy()
            if nan:
                bad[:, k, k] = np.nan
            else:
                bad[0, k, k] -= 2.0 * lkk[k] ** 2
            R, info = tp._run(pk, [good0, bad, good2], words, False)
            print(f"{KERNEL[words]} n={n} k={k} {'NaN' if nan else 'negative'} pivot: info = {info}")
            assert info == [0, k + 1, 0]
            if first is None:
                first = R
                tp._check_factor(KERNEL[words], good0, R[0], words, 0, what="beside a failed block: ")
                tp._check_factor(KERNEL[words], good2, R[2], words, 1, what="beside a failed block: ")
            else:
                assert np.array_equal(np.tril(R[0]), np.tril(first[0]))
                assert np.array_equal(np.tril(R[2]), np.tril(first[2]))


# ---------------------------------------------------------------- past potrf_batched's bound

@pytest.mark.parametrize("kind", [0, 3], ids=["spd", "illcond"])
@pytest.mark.parametrize("words,n", [(1, 1263), (4, 303)], ids=["fp64-1263", "qd-303"])
def test_chain_past_the_old_bound(pk, words, n, kind):
    """One past potrf_batched's largest n (1262 at fp64, 302 at quad-double): CLRSDP_E_ARG
    without the chain, info = 0 and the bound with it (fp64 checked in np.longdouble,
    quad-double in mpmath, as test_gpu_potrf.factor_ratio does)."""
    A = tp._limbs(n, words, kind)
    (L,), info = tp._run(pk, [A], words, False)
    assert info == [0]
    tp._check_factor(KERNEL[words], A, L, words, kind)
    assert not np.triu(L, 1).any()


@WORDS
def test_chain_identity_1500(pk, words):
    """np.eye(1500) factors to the identity, every trailing limb zero."""
    A = np.zeros((words, 1500, 1500))
    A[0] = np.eye(1500)
    (R,), info = tp._run(pk, [A], words, False)
    assert info == [0]
    assert np.array_equal(R[0], np.eye(1500)) and not R[1:].any()


def test_chain_and_one_cu_route_below_the_bound(pk, monkeypatch):
    """fp64 n = 257 by the chain and, with the switch unset, by potrf_batched: both meet the same
    bound.  The two sum an entry's updates in different orders (64 x 64 tiles on the matrix
    cores against one running sum per entry on the VALU), so they agree to rounding and not bitwise."""
    A = tp._limbs(257, 1, 0)
    (Lc,), ic = tp._run(pk, [A], 1, False)
    monkeypatch.delenv("CLRSDP_POTRF_BLK")
    (Lb,), ib = tp._run(pk, [A], 1, False)
    assert ic == [0] and ib == [0]
    tp._check_factor(K64, A, Lc, 1, 0)
    tp._check_factor("potrf_batched<double,16,256>", A, Lb, 1, 0)
    d = float(np.max(np.abs(np.tril(Lc[0]) - np.tril(Lb[0]))) / np.max(np.abs(Lb[0])))
    print(f"chain against potrf_batched, n = 257: max |difference| / max |L| = {d:.3e}")
    assert not np.array_equal(np.tril(Lc), np.tril(Lb))


# ---------------------------------------------------------------- through the solver

QD_SHAPE = dict(delta=40, N=320)
F64_SHAPE = dict(delta=128, N=1280)


def _stage_parity(pk, c, words):
    """every stage of one iteration with the Cholesky factorisations alone (flags 0: no LU
    fallback can stand in for a failed Cholesky) against the fp64 oracle, then the loop body"""
    lul._lu_stage_compare(pk, c, 0, words)
    dev = pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=words)
    try:
        dev.set_factorization(0)
        dev.set_state(*c["state"])
        dev.iterate(pk.make_params("0.3", "0.1", "0.7", 0), False)
        assert dev.factorization == 0
    finally:
        dev.close()


def test_solver_quad_double_dim_S_320(pk, oracle):
    """Quad-double dim_S = 320 > 302 (kappa(S_0) ~ 168, test_gpu_lu_large.py): stage parity with
    the fp64 oracle at 1e-11 with Cholesky alone, one iterate of the loop body, and the dual
    Newton identity Tr(A_* dY) + B dy = d at 1e-50 in 320-bit mpmath."""
    from clrsdp_amd import instance as inst
    c = lul._case(pk, oracle, 4, **QD_SHAPE)
    _stage_parity(pk, c, 4)
    g = _direction_qd(pk, c)
    prec0 = mpmath.mp.prec
    try:
        ar = oracle.Mp(320)
        cons = [pk.Cluster([[[ar.asarray(v) for v in vk] for vk in Al] for Al in cl.A],
                           ar.asarray(cl.B), ar.asarray(cl.c),
                           [[[ar.num(x) for x in hk] for hk in Hl] for Hl in cl.H]) for cl in c["cons"]]
        dY = inst.flat_to_blocks(np.asarray(g["dY"], dtype=object), c["bi"])
        lhs = oracle.trace_A(ar, cons, dY, c["bi"]) + oracle.stack_B(cons) @ np.asarray(g["dy"], dtype=object)
        cmax = max(abs(x) for x in oracle.stack_c(cons))
        err = float(max(abs(a - b) for a, b in zip(lhs, g["d"])) / cmax)
    finally:
        mpmath.mp.prec = prec0
    print(f"dual Newton identity, quad-double dim_S = 320, Cholesky chain: {err:.3e}")
    assert err <= 1e-50


def _direction_qd(pk, c):
    """d and the predictor direction from the exact device buffers (flags 0)"""
    from clrsdp_amd import _lib as L
    P = pk.make_params("0.3", "0.1", "0.7", 0)
    dev = pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=4)
    try:
        dev.set_factorization(0)
        dev.set_state(*c["state"])
        for s in (L.STAGE_MU_R, L.STAGE_XINV, L.STAGE_SCHUR, L.STAGE_FACTOR):
            dev.run_stage(s, P, False)
        dev.run_stage(L.STAGE_RESIDUALS, P, False)
        o = {"d": dev.buffer(L.BUF_DVEC, True)}
        dev.run_stage(L.STAGE_PREDICTOR, P, False)
        for k, bf in (("dy", L.BUF_DY), ("dY", L.BUF_DYMAT)):
            o[k] = dev.buffer(bf, True)
        assert dev.factorization == 0
    finally:
        dev.close()
    return o


def test_solver_fp64_dim_S_1280(pk, oracle):
    """fp64 dim_S = 1280 > 1262 with delta = 128: stage parity with the fp64 oracle at 1e-11
    with Cholesky alone and one iterate of the loop body (X and Y blocks of 128, S_j of 1280 and
    Q all through the chain).  kappa_1(S_0) = 741 (kappa_2 = 86) after the two oracle iterations,
    from the CPU oracle's compute_S_integrated, so the fp64 oracle is a reference to 1e-11; with
    the delta = 64 of test_gpu_lu_large.py's fp64 shape it is 1.2e4 at N = 1280 (delta = 80:
    3.5e3, delta = 96: 1.8e3), past the 1e3 asked of this test.  N <= delta (delta + 1) / 2 =
    8256 holds."""
    c = lul._case(pk, oracle, 1, **F64_SHAPE)
    _stage_parity(pk, c, 1)
