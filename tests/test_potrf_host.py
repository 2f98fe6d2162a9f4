"""clrsdp_potrf (include/clrsdp.h) without a GPU: the symbol is exported and bound, bad arguments
are rejected with CLRSDP_E_ARG before any device work -- and the self-check of the ill-conditioned
inputs of tests/test_gpu_potrf.py (potrf_cases kind 3): the Cholesky recurrence at the word's own
width completes on them with every pivot >= tau, and fails one width lower."""
import ctypes as C

import numpy as np
import pytest

import potrf_cases as pc


def test_potrf_is_exported_and_loads(pk):
    from clrsdp_amd import _lib as L
    assert "clrsdp_potrf" in L.EXPORTS
    fn = L.lib().clrsdp_potrf
    assert fn.restype is C.c_int32
    assert callable(pk.potrf)


BAD = [(3, 0, 4), (1, 0, 0), (2, 0, 0), (1, 0, 4097), (4, 0, 4097), (1, 2, 4), (1, -1, 4),
       (1, 1, 257), (2, 1, 65), (4, 1, 65), (1, 1, 0)]


@pytest.mark.parametrize("words,inverse,n", BAD, ids=[f"w{w}-inv{i}-n{n}" for w, i, n in BAD])
def test_potrf_bad_arguments_are_e_arg_without_a_device(pk, words, inverse, n):
    from clrsdp_amd import _lib as L
    ns = np.array([4, n], dtype=np.int64)          # the bad block is not the first one
    A = np.zeros(8)                                # never read: the checks come first
    info = np.zeros(2, dtype=np.int32)
    # device 1 << 20 does not exist anywhere: an argument check that came after the device work
    # would report CLRSDP_E_HIP instead
    rc = L.lib().clrsdp_potrf(1 << 20, words, inverse, 2, ns.ctypes.data_as(L.P_i64),
                              A.ctypes.data_as(L.P_f64), info.ctypes.data_as(L.P_i32))
    assert rc == L.E_ARG


def test_potrf_null_and_empty_are_e_arg(pk):
    from clrsdp_amd import _lib as L
    ns = np.array([4], dtype=np.int64)
    A = np.zeros(16)
    info = np.zeros(1, dtype=np.int32)
    p = (ns.ctypes.data_as(L.P_i64), A.ctypes.data_as(L.P_f64), info.ctypes.data_as(L.P_i32))
    for inverse in (0, 1):
        assert L.lib().clrsdp_potrf(0, 1, inverse, 0, *p) == L.E_ARG
        assert L.lib().clrsdp_potrf(0, 1, inverse, -1, *p) == L.E_ARG
        assert L.lib().clrsdp_potrf(0, 1, inverse, 1, None, p[1], p[2]) == L.E_ARG
        assert L.lib().clrsdp_potrf(0, 1, inverse, 1, p[0], None, p[2]) == L.E_ARG
        assert L.lib().clrsdp_potrf(0, 1, inverse, 1, p[0], p[1], None) == L.E_ARG


def test_solver_potrf_rejects_non_square(pk):
    with pytest.raises(ValueError):
        pk.potrf([np.zeros((3, 4))])
    with pytest.raises(ValueError):
        pk.potrf([np.zeros((2, 3, 4))], precision_words=2)
    with pytest.raises(ValueError):
        pk.potrf([np.zeros((1, 3, 3))], precision_words=2)     # one limb where two are due


# ---- the ill-conditioned inputs (kind 3) need the word's full width

def _kind3(pk, n, words):
    from clrsdp_amd import instance as inst
    return pc.spd_limbs(inst, n, words, 3)


def test_kind3_is_exactly_representable(pk):
    """the limbs are a normalised multi-word number (|limb q+1| <= ulp(limb q) / 2) and symmetric"""
    for words in (1, 2, 4):
        A = _kind3(pk, 96, words)
        assert np.array_equal(A, A.transpose(0, 2, 1))
        if words > 1:
            assert np.array_equal(A[0], np.rint(A[0]))
            assert np.all(np.abs(A[1]) <= 0.5 * np.spacing(np.abs(A[0])))
            assert np.array_equal(np.diag(A[1]), np.full(96, pc.TAU[words])) and not A[2:].any()


@pytest.mark.parametrize("n", [64, 96, 129, 256])
def test_kind3_factors_at_53_bits(pk, n):
    fail, pmin = pc.cholesky_at(_kind3(pk, n, 1), 53)
    print(f"kind 3 fp64 n={n}: smallest pivot / tau = {pmin / pc.TAU[1]:.3f}")
    assert fail == 0 and pmin >= pc.TAU[1]


@pytest.mark.parametrize("n", [64, 96, 129])
@pytest.mark.parametrize("words", [2, 4], ids=["dd", "qd"])
def test_kind3_needs_the_full_word(pk, words, n):
    """At the word's own precision (104 / 206 bits) the recurrence completes with every pivot
    >= tau; one width lower (53 / 104 bits) the same matrix fails: a kernel that rounds a pivot
    or an update to the narrower width cannot return info = 0 on it."""
    A = _kind3(pk, n, words)
    fail, pmin = pc.cholesky_at(A, pc.BITS[words])
    lower = {2: 53, 4: 104}[words]
    fail_lo, _ = pc.cholesky_at(A, lower)
    print(f"kind 3 words={words} n={n}: smallest pivot / tau = {float(pmin / pc.TAU[words]):.3f} at "
          f"{pc.BITS[words]} bits; at {lower} bits the recurrence fails at column {fail_lo}")
    assert fail == 0 and pmin >= pc.TAU[words]
    assert fail_lo > 0
