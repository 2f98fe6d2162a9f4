"""solver.potrf_kernel (clrsdp_potrf_kernel, a host-only query: no device, no launch) returns the
route MatPlan::potrf takes per word width, largest block and the three-state CLRSDP_POTRF_BLK
(MatPlan<T>::potrf_dispatch, the one place that decides it)."""
import ctypes as C

import pytest

BATCHED, LA64, LA128, BLK, BLK64 = range(5)   # CLRSDP_POTRF_K_* (include/clrsdp.h)
SIZES = (1, 64, 65, 128, 129, 4096)
# (words, switch) -> the route at nmax <= 64, 65 .. 128, >= 129
ROWS = {
    (1, None): (BATCHED, BATCHED, BATCHED), (1, "0"): (BATCHED, BATCHED, BATCHED),
    (1, "1"): (BLK64, BLK64, BLK64),
    (2, None): (LA64, BLK, BLK), (2, "1"): (LA64, BLK, BLK),
    (2, "0"): (LA64, LA128, BATCHED),
    (4, None): (LA64, BATCHED, BATCHED), (4, "0"): (LA64, BATCHED, BATCHED),
    (4, "1"): (LA64, BLK, BLK),
}


@pytest.mark.parametrize("value", [None, "0", "1"])
@pytest.mark.parametrize("words", [1, 2, 4])
def test_table(pk, monkeypatch, words, value):
    if value is None:
        monkeypatch.delenv("CLRSDP_POTRF_BLK", raising=False)
    else:
        monkeypatch.setenv("CLRSDP_POTRF_BLK", value)
    want = {n: ROWS[(words, value)][0 if n <= 64 else 1 if n <= 128 else 2] for n in SIZES}
    assert {n: pk.potrf_kernel(n, words) for n in SIZES} == want


def test_on_is_anything_not_starting_with_0(pk, monkeypatch):
    monkeypatch.setenv("CLRSDP_POTRF_BLK", "yes")
    assert pk.potrf_kernel(300, 1) == BLK64 and pk.potrf_kernel(300, 4) == BLK
    monkeypatch.setenv("CLRSDP_POTRF_BLK", "00")
    assert pk.potrf_kernel(300, 1) == BATCHED and pk.potrf_kernel(100, 2) == LA128


def test_arguments_are_checked(pk, monkeypatch):
    from clrsdp_amd import _lib
    monkeypatch.delenv("CLRSDP_POTRF_BLK", raising=False)
    for words, nmax in ((3, 10), (1, 0), (1, 4097)):
        with pytest.raises(_lib.ClrsdpError) as e:
            pk.potrf_kernel(nmax, words)
        assert e.value.code == _lib.E_ARG
    assert _lib.lib().clrsdp_potrf_kernel(1, 10, None) == _lib.E_ARG
    k = C.c_int32(-1)
    assert _lib.lib().clrsdp_potrf_kernel(1, 10, C.byref(k)) == _lib.OK and k.value == BATCHED
    assert (_lib.POTRF_K_BATCHED, _lib.POTRF_K_LA64, _lib.POTRF_K_LA128, _lib.POTRF_K_BLK,
            _lib.POTRF_K_BLK64) == (BATCHED, LA64, LA128, BLK, BLK64)
