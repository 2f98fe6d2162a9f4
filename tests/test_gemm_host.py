"""clrsdp_gemm / clrsdp_gemm_chain (include/clrsdp.h) without a GPU:
  1. both symbols are exported and bound, and every refusal of the header is CLRSDP_E_ARG before
     any device work (device 1 << 20 exists nowhere; the bad problem is not the first one);
  2. the reference of tests/gemm_cases.py holds on its own: numpy's fp64 product meets the fp64
     bound on every class, the exact product agrees with a direct 320-bit triple loop, the limb
     split round-trips, the cancelling class cancels;
  3. sensitivity: each way a kernel could be subtly wrong, applied to the reference result, exceeds
     the bound on every operand class at every width -- what the GPU tests would notice."""
import ctypes as C

import mpmath
import numpy as np
import pytest

import gemm_cases as gc
from helpers import _exact_ints, cw_err

NO_DEVICE = 1 << 20
WORDS = [1, 2, 4]


# ---- 1. symbols and argument checks -------------------------------------------------------------
def test_symbols_are_exported_and_bound(pk):
    from clrsdp_amd import _lib as L
    for name in ("clrsdp_gemm", "clrsdp_gemm_chain"):
        assert name in L.EXPORTS
        assert getattr(L.lib(), name).restype is C.c_int32
    assert callable(pk.gemm) and callable(pk.gemm_chain)
    assert C.sizeof(L.GemmProblem) == 12 * 8 + 4 * 4 + 2 * 8


def _recs(L, second, first=None):
    """two 4 x 4 x 4 problems in arenas of 64 numbers per buffer; `second` overrides fields of the
    second one"""
    r = (L.GemmProblem * 2)()
    for p, over in enumerate((first or {}, second)):
        f = dict(M=4, N=4, K=4, lda=4, ldb=4, ldc=4, ldcin=4, offa=16 * p, offb=16 * p, offc=16 * p,
                 offcin=16 * p, offs=4 * p)
        f.update(over)
        for k, v in f.items():
            setattr(r[p], k, v)
    return r


def _gemm(L, recs, words=1, form=0, ta=0, tb=0, alpha=1.0, beta=0.0, dscal=False, cin=True, sa=True,
          null=(), nprob=2, n=64):
    buf = {k: np.zeros(4 * n) for k in ("A", "B", "C", "Cin", "sa", "sl")}   # never read
    ptr = {k: (None if k in null else v.ctypes.data_as(L.P_f64)) for k, v in buf.items()}
    ds = np.ones(1)
    path = C.c_int32(-1)
    rc = L.lib().clrsdp_gemm(NO_DEVICE, words, form, ta, tb, alpha, beta,
                             ds.ctypes.data_as(L.P_f64) if dscal else None, 1.0, nprob,
                             None if "prob" in null else recs, ptr["A"], n, ptr["B"], n, ptr["C"], n,
                             ptr["Cin"] if cin else None, n, ptr["sa"] if sa else None,
                             ptr["sl"] if sa else None, n, C.byref(path))
    assert path.value == -1
    return rc


def test_a_good_call_reaches_the_device(pk):
    """the checks pass, the device does not exist: CLRSDP_E_HIP, for each form"""
    from clrsdp_amd import _lib as L
    assert _gemm(L, _recs(L, {})) == L.E_HIP
    assert _gemm(L, _recs(L, {}), form=L.GEMM_SYM, tb=1) == L.E_HIP
    assert _gemm(L, _recs(L, {}), form=L.GEMM_UPPER, words=2) == L.E_HIP
    assert _gemm(L, _recs(L, {}), form=L.GEMM_SCALED, tb=1) == L.E_HIP
    assert _gemm(L, _recs(L, dict(diag=1, alpha=1.0)), form=L.GEMM_MIXED, dscal=True) == L.E_HIP
    assert _gemm(L, _recs(L, {}), beta=0.5) == L.E_HIP
    assert _gemm(L, _recs(L, {}), beta=0.5, cin=False) == L.E_HIP


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("field", ["M", "N", "K"])
@pytest.mark.parametrize("v", [0, -1, 4097])
def test_sizes_out_of_range(pk, words, field, v):
    from clrsdp_amd import _lib as L
    assert _gemm(L, _recs(L, {field: v}), words=words) == L.E_ARG


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_leading_dimension_below_the_stored_rows(pk, ta, tb):
    from clrsdp_amd import _lib as L
    shape = dict(M=3, N=2, K=5, offa=16, offb=32, offc=16)
    ar, br = (5 if ta else 3), (2 if tb else 5)
    good = dict(shape, lda=ar, ldb=br, ldc=3, ldcin=3)
    assert _gemm(L, _recs(L, good), ta=ta, tb=tb, beta=0.5) == L.E_HIP
    for k, rows in (("lda", ar), ("ldb", br), ("ldc", 3), ("ldcin", 3)):
        assert _gemm(L, _recs(L, dict(good, **{k: rows - 1})), ta=ta, tb=tb, beta=0.5) == L.E_ARG, k
    # C_in is not read with beta = 0, and ldcin not used in place
    assert _gemm(L, _recs(L, dict(good, ldcin=1)), ta=ta, tb=tb) == L.E_HIP
    assert _gemm(L, _recs(L, dict(good, ldcin=1, offcin=-1)), ta=ta, tb=tb, beta=0.5) == L.E_HIP


def test_forms_and_widths(pk):
    from clrsdp_amd import _lib as L
    sq = _recs(L, {})
    for words in (2, 4):
        assert _gemm(L, sq, words=words, form=L.GEMM_SYM, tb=1) == L.E_ARG
        assert _gemm(L, sq, words=words, form=L.GEMM_SCALED, tb=1) == L.E_ARG
        assert _gemm(L, sq, words=words, form=L.GEMM_MIXED) == L.E_ARG
        assert _gemm(L, sq, words=words, dscal=True) == L.E_ARG
    assert _gemm(L, sq, words=1, form=L.GEMM_UPPER) == L.E_ARG
    for words in (0, 3, 8):
        assert _gemm(L, sq, words=words) == L.E_ARG
    for form in (-1, 5):
        assert _gemm(L, sq, form=form) == L.E_ARG
    # SYM / UPPER: square only (the second problem is 4 x 3)
    rect = _recs(L, dict(N=3))
    assert _gemm(L, rect, form=L.GEMM_SYM, tb=1) == L.E_ARG
    assert _gemm(L, rect, form=L.GEMM_UPPER, words=2) == L.E_ARG
    # SYM: op(A) = A, beta = 0, no diagonal scalar
    assert _gemm(L, sq, form=L.GEMM_SYM, ta=1) == L.E_ARG
    assert _gemm(L, sq, form=L.GEMM_SYM, beta=1.0) == L.E_ARG
    assert _gemm(L, sq, form=L.GEMM_SYM, dscal=True) == L.E_ARG
    # SCALED: A B^T only, with both factor vectors
    for ta, tb in ((0, 0), (1, 0), (1, 1)):
        assert _gemm(L, sq, form=L.GEMM_SCALED, ta=ta, tb=tb) == L.E_ARG
    assert _gemm(L, sq, form=L.GEMM_SCALED, tb=1, sa=False) == L.E_ARG
    # MIXED diag: square, with the scalar
    assert _gemm(L, _recs(L, dict(diag=1)), form=L.GEMM_MIXED) == L.E_ARG
    assert _gemm(L, _recs(L, dict(diag=1, N=3)), form=L.GEMM_MIXED, dscal=True) == L.E_ARG
    # the diagonal scalar with a batch of matrix-vector products
    assert _gemm(L, _recs(L, dict(N=1), first=dict(N=1)), dscal=True) == L.E_ARG


def test_offsets(pk):
    from clrsdp_amd import _lib as L
    for over in (dict(offc=15), dict(offc=0), dict(offc=12, ldc=5)):      # C regions overlap
        assert _gemm(L, _recs(L, over)) == L.E_ARG, over
    assert _gemm(L, _recs(L, dict(offc=12, ldc=5), first=dict(offc=40))) == L.E_HIP
    for k in ("offa", "offb", "offc"):                                   # outside the arena
        assert _gemm(L, _recs(L, {k: 49})) == L.E_ARG, k
        assert _gemm(L, _recs(L, {k: -1})) == L.E_ARG, k
    assert _gemm(L, _recs(L, dict(offcin=49)), beta=1.0) == L.E_ARG
    assert _gemm(L, _recs(L, dict(offs=61)), form=L.GEMM_SCALED, tb=1) == L.E_ARG
    assert _gemm(L, _recs(L, dict(lda=1 << 25))) == L.E_ARG


def test_null_and_empty(pk):
    from clrsdp_amd import _lib as L
    for k in ("prob", "A", "B", "C"):
        assert _gemm(L, _recs(L, {}), null=(k,)) == L.E_ARG, k
    assert _gemm(L, _recs(L, {}), nprob=0) == L.E_ARG
    assert _gemm(L, _recs(L, {}), nprob=-1) == L.E_ARG


def _chain(L, form=0, n=4, nprob=2, halves=1, ncols=0, null=(), dot=False):
    names = ("A1", "B1", "C1", "A2", "O", "DA", "DdA", "DB", "dot", "lam", "din", "rout")
    buf = {k: np.zeros(256) for k in names}
    p = {k: (None if k in null else v.ctypes.data_as(L.P_f64)) for k, v in buf.items()}
    if not dot:
        p["dot"] = None
    return L.lib().clrsdp_gemm_chain(NO_DEVICE, form, n, nprob, halves, ncols, 1.0, -1.0, p["A1"],
                                     p["B1"], p["C1"], p["A2"], p["O"], p["DA"], p["DdA"], p["DB"],
                                     p["dot"], p["lam"], p["din"], 1.0, 1.0, p["rout"])


def test_chain_refusals(pk):
    from clrsdp_amd import _lib as L
    assert _chain(L) == L.E_HIP
    assert _chain(L, form=L.CHAIN_SYM, halves=2, nprob=1) == L.E_HIP
    assert _chain(L, form=L.CHAIN_TRACE, ncols=3) == L.E_HIP
    for n in (129, 0, -1, 4096):
        for form in (L.CHAIN, L.CHAIN_SYM, L.CHAIN_TRACE):
            assert _chain(L, form=form, n=n, ncols=3) == L.E_ARG
    for form in (-1, 3):
        assert _chain(L, form=form) == L.E_ARG
    assert _chain(L, nprob=0) == L.E_ARG
    assert _chain(L, halves=2) == L.E_ARG                  # two pointer sets: CHAIN_SYM only
    assert _chain(L, form=L.CHAIN_SYM, halves=3) == L.E_ARG
    assert _chain(L, form=L.CHAIN_TRACE, ncols=0) == L.E_ARG
    assert _chain(L, form=L.CHAIN_TRACE, ncols=4097) == L.E_ARG
    for k in ("A1", "B1", "A2", "O"):
        assert _chain(L, null=(k,)) == L.E_ARG, k
    assert _chain(L, null=("C1", "din")) == L.E_HIP         # both optional
    for k in ("DA", "DdA", "DB"):
        assert _chain(L, null=(k,), dot=True) == L.E_ARG, k
    for k in ("A1", "B1", "lam", "rout"):
        assert _chain(L, form=L.CHAIN_TRACE, ncols=3, null=(k,)) == L.E_ARG, k


def test_python_wrappers_reject_bad_shapes(pk):
    z = np.zeros
    with pytest.raises(ValueError):
        pk.gemm([z((3, 4))], [z((5, 2))])                    # inner dimensions differ
    with pytest.raises(ValueError):
        pk.gemm([z((3, 4))], [])
    with pytest.raises(ValueError):
        pk.gemm([z((3, 4))], [z((4, 2))], form="banded")
    with pytest.raises(ValueError):
        pk.gemm([z((3, 4))], [z((4, 2))], Cin=[z((3, 3))], beta=1.0)
    with pytest.raises(ValueError):
        pk.gemm([z((3, 4))], [z((4, 2))], form="mixed")
    with pytest.raises(ValueError):
        pk.gemm([z((3, 4))], [z((2, 4))], form="scaled", transb=True, sa=[z(3)], sl=[z(4)])
    with pytest.raises(ValueError):
        pk.gemm([z((2, 3, 4))], [z((4, 2))], precision_words=4)    # raw limbs of the wrong width
    with pytest.raises(ValueError):
        pk.gemm_chain("chain", [z((3, 4))], [z((3, 3))], [z((3, 3))])
    with pytest.raises(ValueError):
        pk.gemm_chain("chain", [z((3, 3))], [z((4, 4))], [z((3, 3))])
    with pytest.raises(ValueError):
        pk.gemm_chain("trace", [z((3, 3))], [z((3, 5))], lam=[z(4)])
    with pytest.raises(ValueError):
        pk.gemm_chain("sym", [z((3, 3))] * 3, [z((3, 3))] * 3, halves=2)


# ---- 2. the reference holds on its own ----------------------------------------------------------
SHAPE = (20, 19, 37)          # M >= 16, N >= 8 (the tile mutation), K > 32 (the k = 32 mutation), K odd
ALPHA, BETA, DIAG = 2.0, 0.5, -0.75


@pytest.mark.parametrize("kind", gc.KINDS)
def test_numpy_fp64_meets_the_fp64_bound(pk, kind):
    """float64 matmul is one of the admissible evaluation orders: ratio <= 1 on every class, with
    C_in and the diagonal term, and on the scaled-A form with its own constant"""
    for M, N, K in (SHAPE, (1, 1, 1), (65, 63, 130), (7, 1, 260)):
        A, B = gc.operands(kind, M, N, K, 1, seed=3)
        Cin = gc.matrix(kind, M, N, 1, seed=3)
        got = ALPHA * (A[0] @ B[0]) + BETA * Cin[0] + DIAG * np.eye(M, N)
        ref = gc.reference(gc.product(A, B), ALPHA, BETA, Cin, DIAG)
        r = gc.ratio(got[None], ref, gc.bound(A, B, 1, ALPHA, BETA, Cin, DIAG))
        assert r <= 1.0, (kind, M, N, K, r)
        s = gc._uniform(4, 70, (K,)) * gc._uniform(4, 71, (K,))
        got = (A[0] * s[None, :]) @ B[0]
        ref = gc.reference(gc.product(A, B, scale=s))
        r = gc.ratio(got[None], ref, gc.bound(A, B, 1, extra=6, scale=s))
        assert r <= 1.0, (kind, "scaled", M, N, K, r)


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("kind", gc.KINDS)
def test_exact_product_against_a_direct_triple_loop(pk, kind, words):
    M, N, K = 5, 4, 7
    A, B = gc.operands(kind, M, N, K, words, seed=9)
    ref = gc.reference(gc.product(A, B))
    with mpmath.workprec(gc.PREC):
        Am, Bm = gc.limb_sum(A), gc.limb_sum(B)
        for i in range(M):
            for j in range(N):
                s, sa = mpmath.mpf(0), mpmath.mpf(0)
                for k in range(K):
                    s += Am[i, k] * Bm[k, j]
                    sa += abs(Am[i, k] * Bm[k, j])
                assert abs(s - ref[i, j]) <= mpmath.ldexp(sa, -300), (i, j)


@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("kind", gc.KINDS)
def test_limbs_round_trip_and_integers_agree(pk, kind, words):
    A, B = gc.operands(kind, 6, 5, 9, words, seed=12)
    for X in (A, B, gc.matrix(kind, 6, 5, words, seed=12)):
        assert np.array_equal(gc.split(gc.limb_sum(X), words), X)
        I, e = gc.ints(X)
        with mpmath.workprec(1200):
            S = sum(np.frompyfunc(mpmath.mpf, 1, 1)(X[q]) for q in range(words))
            J, f = _exact_ints(S)
        g = min(e, f)
        assert np.array_equal(I << (e - g), J << (f - g))
    if kind != "exact":        # every limb is filled, the last term, row and column are nonzero
        assert np.all(A != 0.0) and np.all(B != 0.0)


@pytest.mark.parametrize("words", WORDS)
def test_the_cancelling_class_cancels(pk, words):
    for M, N, K in (SHAPE, (9, 8, 2), (8, 9, 3), (17, 17, 64)):
        A, B = gc.operands("cancel", M, N, K, words, seed=7)
        with mpmath.workprec(gc.PREC):
            P = gc.reference(gc.product(A, B))
            for i in range(M):
                for j in range(N):
                    assert abs(P[i, j]) <= 2.0 ** -30 * float(gc.abs1(A)[i] @ gc.abs1(B)[:, j])


# ---- 3. sensitivity -----------------------------------------------------------------------------
_cases = {}


def _case(kind, words):
    if (kind, words) not in _cases:
        M, N, K = SHAPE
        A, B = gc.operands(kind, M, N, K, words, seed=5)
        Cin = gc.matrix(kind, M, N, words, seed=5)
        diag = DIAG if words == 1 else 0.0            # (the diagonal scalar is fp64 only)
        ref = gc.reference(gc.product(A, B), ALPHA, BETA, Cin, diag)
        bnd = gc.bound(A, B, words, ALPHA, BETA, Cin, diag)
        _cases[(kind, words)] = (A, B, Cin, diag, ref, bnd)
    return _cases[(kind, words)]


def _mutate(name, A, B, Cin, diag, ref):
    """the result a kernel with the named defect would have produced, exactly"""
    K = A.shape[2]
    rebuilt = lambda A2, B2, C2=Cin, d=diag: gc.reference(gc.product(A2, B2), ALPHA, BETA, C2, d)
    if name == "drop_last_k":
        return rebuilt(A[:, :, :K - 1], B[:, :K - 1, :])
    if name == "drop_k32":
        return rebuilt(np.delete(A, 32, axis=2), np.delete(B, 32, axis=1))
    if name == "zero_low_limb":
        A2 = A.copy()
        i, k = A.shape[1] - 1, 0
        q = max(q for q in range(A.shape[0]) if A[q, i, k] != 0.0)
        A2[q, i, k] = 0.0
        return rebuilt(A2, B)
    if name == "neighbour_cin":
        return rebuilt(A, B, np.roll(Cin, 1, axis=1))
    if name == "transposed_tile":
        m = ref.copy()
        m[8:16, 0:8] = ref[8:16, 0:8].T
        return m
    if name == "no_diagonal_scalar":
        return rebuilt(A, B, Cin, 0.0)
    raise ValueError(name)


MUTATIONS = ["drop_last_k", "drop_k32", "zero_low_limb", "neighbour_cin", "transposed_tile"]


@pytest.mark.parametrize("name", MUTATIONS)
@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("kind", gc.KINDS)
def test_a_wrong_kernel_would_exceed_the_bound(pk, kind, words, name):
    A, B, Cin, diag, ref, bnd = _case(kind, words)
    assert cw_err(ref, ref, bnd) == 0.0
    r = cw_err(_mutate(name, A, B, Cin, diag, ref), ref, bnd)
    assert r > 1.0, (kind, words, name, r)


@pytest.mark.parametrize("kind", gc.KINDS)
def test_a_missing_diagonal_scalar_would_exceed_the_bound(pk, kind):
    """(the diagonal scalar exists at fp64 only)"""
    A, B, Cin, diag, ref, bnd = _case(kind, 1)
    assert diag != 0.0
    r = cw_err(_mutate("no_diagonal_scalar", A, B, Cin, diag, ref), ref, bnd)
    assert r > 1.0, (kind, r)


@pytest.mark.parametrize("n", [33, 48, 128])
def test_sym_chain_reference_notices_a_nonzero_above_the_diagonal(pk, n):
    """chain_f64's SYM form never reads L above the diagonal; were an entry there nonzero, the
    true L M L^T would differ from what it computes by more than the bound"""
    L, M = gc.known_lower(n, seed=8), gc.sym_matrix(n, seed=8)
    assert np.all(np.triu(L, 1) == 0.0)
    ref, bnd = gc.congruence_reference(L, M)
    Lbad = L.copy()
    Lbad[2, n - 1] = L[2, 2]
    bad, _ = gc.congruence_reference(Lbad, M)
    assert cw_err(bad, ref, bnd) > 1.0
    assert np.all(ref == ref.T)                      # the exact congruence is symmetric
