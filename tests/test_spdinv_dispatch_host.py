"""solver.spdinv_kernel (clrsdp_spdinv_kernel, a host-only query: no device, no launch) returns
the rule by which the XINV stage and chol(Q) form the inverse inside chol_inv_tiles' launch
(CholInvPlan::spdinv_dispatch): fp64 and nmax <= 128 only, never with the pivoted-LU fallback
(lu_x() for X, lu_sq() for Q), and CLRSDP_CHOL_SPDINV=0 keeps the GEMM everywhere."""
import pytest

# (words, nmax, lu) -> fused, the switch at its default
TABLE = {
    (1, 1, False): True, (1, 32, False): True, (1, 33, False): True, (1, 64, False): True,
    (1, 65, False): True, (1, 128, False): True, (1, 129, False): False, (1, 256, False): False,
    (1, 4096, False): False,
    (1, 1, True): False, (1, 64, True): False, (1, 128, True): False, (1, 129, True): False,
    (2, 1, False): False, (2, 64, False): False, (2, 128, False): False, (2, 32, True): False,
    (4, 1, False): False, (4, 32, False): False, (4, 64, False): False, (4, 18, True): False,
}


@pytest.mark.parametrize("value", [None, "1"])
def test_table_with_the_switch_on(pk, monkeypatch, value):
    if value is None:
        monkeypatch.delenv("CLRSDP_CHOL_SPDINV", raising=False)
    else:
        monkeypatch.setenv("CLRSDP_CHOL_SPDINV", value)
    got = {k: pk.spdinv_kernel(k[1], k[0], k[2]) for k in TABLE}
    assert got == TABLE


def test_switch_off_keeps_the_gemm_everywhere(pk, monkeypatch):
    monkeypatch.setenv("CLRSDP_CHOL_SPDINV", "0")
    for words in (1, 2, 4):
        for lu in (False, True):
            for nmax in range(1, 300):
                assert not pk.spdinv_kernel(nmax, words, lu), (words, nmax, lu)


def test_boundary_is_exactly_128_at_fp64(pk, monkeypatch):
    monkeypatch.delenv("CLRSDP_CHOL_SPDINV", raising=False)
    for nmax in range(1, 300):
        assert pk.spdinv_kernel(nmax, 1) == (nmax <= 128), nmax
        assert not pk.spdinv_kernel(nmax, 1, True), nmax


def test_arguments_are_checked(pk):
    for words, nmax in ((3, 10), (1, 0), (1, 4097)):
        with pytest.raises(Exception):
            pk.spdinv_kernel(nmax, words)
