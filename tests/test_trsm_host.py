"""clrsdp_trsm (include/clrsdp.h) without a GPU: the symbol is exported and bound, and bad
arguments are rejected with CLRSDP_E_ARG before any device work."""
import ctypes as C

import numpy as np
import pytest

# device 1 << 20 does not exist anywhere: an argument check that came after the device work would
# report CLRSDP_E_HIP instead
NO_DEVICE = 1 << 20


def test_trsm_is_exported_and_loads(pk):
    from clrsdp_amd import _lib as L
    assert "clrsdp_trsm" in L.EXPORTS
    fn = L.lib().clrsdp_trsm
    assert fn.restype is C.c_int32
    assert callable(pk.trsm)


def _call(L, words, mode, ns, nrhs=(1, 1)):
    ns = np.array(ns, dtype=np.int64)
    nr = np.array(nrhs, dtype=np.int64)
    A = np.zeros(64)                               # never read: the checks come first
    B = np.zeros(64)
    return L.lib().clrsdp_trsm(NO_DEVICE, words, mode, 0, 2, ns.ctypes.data_as(L.P_i64),
                               nr.ctypes.data_as(L.P_i64), A.ctypes.data_as(L.P_f64),
                               B.ctypes.data_as(L.P_f64))


@pytest.mark.parametrize("words", [0, 3, 5, 8])
def test_trsm_bad_words_are_e_arg_without_a_device(pk, words):
    from clrsdp_amd import _lib as L
    assert _call(L, words, 0, [4, 4]) == L.E_ARG


@pytest.mark.parametrize("mode", [-1, 3])
def test_trsm_bad_mode_is_e_arg_without_a_device(pk, mode):
    from clrsdp_amd import _lib as L
    assert _call(L, 1, mode, [4, 4]) == L.E_ARG


@pytest.mark.parametrize("words", [1, 2, 4])
@pytest.mark.parametrize("n", [0, -1, 4097])
def test_trsm_bad_sizes_are_e_arg_without_a_device(pk, words, n):
    from clrsdp_amd import _lib as L
    assert _call(L, words, 1, [4, n]) == L.E_ARG          # the bad block is not the first one
    assert _call(L, words, 1, [4, 4], nrhs=(1, n)) == L.E_ARG


def test_trsm_null_and_empty_are_e_arg(pk):
    from clrsdp_amd import _lib as L
    ns = np.array([4], dtype=np.int64)
    nr = np.array([1], dtype=np.int64)
    A = np.zeros(16)
    B = np.zeros(4)
    p = [ns.ctypes.data_as(L.P_i64), nr.ctypes.data_as(L.P_i64), A.ctypes.data_as(L.P_f64),
         B.ctypes.data_as(L.P_f64)]
    f = L.lib().clrsdp_trsm
    assert f(NO_DEVICE, 1, 0, 0, 0, *p) == L.E_ARG
    for k in range(4):
        q = list(p)
        q[k] = None
        assert f(NO_DEVICE, 1, 0, 0, 1, *q) == L.E_ARG


def test_solver_trsm_rejects_bad_shapes(pk):
    with pytest.raises(ValueError):
        pk.trsm([np.zeros((3, 4))], [np.zeros(3)], 0, False)
    with pytest.raises(ValueError):
        pk.trsm([np.zeros((3, 3))], [np.zeros(4)], 0, False)
    with pytest.raises(ValueError):
        pk.trsm([np.zeros((3, 3))], [], 0, False)
