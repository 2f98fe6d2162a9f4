"""clrsdp_getrf (include/clrsdp.h) without a GPU: the symbol is exported and bound, and bad
arguments are rejected with CLRSDP_E_ARG before any device work."""
import ctypes as C

import numpy as np
import pytest


def test_getrf_is_exported_and_loads(pk):
    from clrsdp_amd import _lib as L
    assert "clrsdp_getrf" in L.EXPORTS
    fn = L.lib().clrsdp_getrf
    assert fn.restype is C.c_int32
    assert callable(pk.getrf)


@pytest.mark.parametrize("words,n", [(3, 4), (1, 0), (2, 0), (1, 4097), (4, 4097)],
                         ids=["words3", "n0-fp64", "n0-dd", "n4097-fp64", "n4097-qd"])
def test_getrf_bad_arguments_are_e_arg_without_a_device(pk, words, n):
    from clrsdp_amd import _lib as L
    ns = np.array([4, n], dtype=np.int64)          # the bad block is not the first one
    A = np.zeros(8)                                # never read: the checks come first
    perm = np.zeros(8, dtype=np.int32)
    info = np.zeros(2, dtype=np.int32)
    # device 1 << 20 does not exist anywhere: an argument check that came after the device work
    # would report CLRSDP_E_HIP instead
    rc = L.lib().clrsdp_getrf(1 << 20, words, 2, ns.ctypes.data_as(L.P_i64),
                              A.ctypes.data_as(L.P_f64), perm.ctypes.data_as(L.P_i32),
                              info.ctypes.data_as(L.P_i32))
    assert rc == L.E_ARG


def test_getrf_null_and_empty_are_e_arg(pk):
    from clrsdp_amd import _lib as L
    ns = np.array([4], dtype=np.int64)
    A = np.zeros(16)
    perm = np.zeros(4, dtype=np.int32)
    info = np.zeros(1, dtype=np.int32)
    p = (ns.ctypes.data_as(L.P_i64), A.ctypes.data_as(L.P_f64), perm.ctypes.data_as(L.P_i32),
         info.ctypes.data_as(L.P_i32))
    assert L.lib().clrsdp_getrf(0, 1, 0, *p) == L.E_ARG
    assert L.lib().clrsdp_getrf(0, 1, 1, p[0], None, p[2], p[3]) == L.E_ARG
    assert L.lib().clrsdp_getrf(0, 1, 1, p[0], p[1], None, p[3]) == L.E_ARG
    assert L.lib().clrsdp_getrf(0, 1, 1, p[0], p[1], p[2], None) == L.E_ARG


def test_solver_getrf_rejects_non_square(pk):
    with pytest.raises(ValueError):
        pk.getrf([np.zeros((3, 4))])
