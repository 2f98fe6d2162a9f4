"""solver.eigmin_kernel (clrsdp_eigmin_kernel, a host-only query: no device, no launch) returns
the dispatch table of MatPlan<T>::eigmin -- the table of test_gpu_eigmin_sizes.py's docstring --
on both sides of every boundary; CLRSDP_EIG_BLK unset and 0 give the same table, and with 1 the
eigblk_* chain stands exactly where eigmin_batched stood and nowhere else."""
import pytest

SPLIT, MX, LDS2, LDS, BATCHED, BLK = range(6)   # CLRSDP_EIG_K_* (include/clrsdp.h)

# (words, nmax) -> kernel, the switch off
TABLE = {
    (1, 1): SPLIT, (1, 128): SPLIT, (1, 129): LDS, (1, 138): LDS, (1, 139): BATCHED, (1, 4096): BATCHED,
    (2, 1): MX, (2, 64): MX, (2, 65): LDS2, (2, 93): LDS2, (2, 94): LDS, (2, 96): LDS, (2, 97): BATCHED,
    (2, 4096): BATCHED,
    (4, 1): MX, (4, 64): MX, (4, 65): LDS, (4, 66): LDS, (4, 67): BATCHED, (4, 4096): BATCHED,
}


@pytest.mark.parametrize("value", [None, "0"])
def test_table_with_the_switch_off(pk, monkeypatch, value):
    monkeypatch.delenv("CLRSDP_EIG_MX", raising=False)
    if value is None:
        monkeypatch.delenv("CLRSDP_EIG_BLK", raising=False)
    else:
        monkeypatch.setenv("CLRSDP_EIG_BLK", value)
    got = {k: pk.eigmin_kernel(k[1], k[0]) for k in TABLE}
    assert got == TABLE


def test_chain_stands_where_eigmin_batched_stood(pk, monkeypatch):
    monkeypatch.delenv("CLRSDP_EIG_MX", raising=False)
    monkeypatch.setenv("CLRSDP_EIG_BLK", "1")
    for words in (1, 2, 4):
        for nmax in range(1, 300):
            monkeypatch.setenv("CLRSDP_EIG_BLK", "1")
            on = pk.eigmin_kernel(nmax, words)
            monkeypatch.delenv("CLRSDP_EIG_BLK")
            off = pk.eigmin_kernel(nmax, words)
            assert on == (BLK if off == BATCHED else off), (words, nmax, on, off)
    monkeypatch.setenv("CLRSDP_EIG_BLK", "1")
    want = {k: (BLK if v == BATCHED else v) for k, v in TABLE.items()}
    assert {k: pk.eigmin_kernel(k[1], k[0]) for k in TABLE} == want


def test_arguments_are_checked(pk):
    from clrsdp_amd import _lib
    for words, nmax in ((3, 10), (1, 0), (1, 4097)):
        with pytest.raises(Exception):
            pk.eigmin_kernel(nmax, words)
    assert _lib.EIG_K_BLK == BLK and _lib.EIG_K_BATCHED == BATCHED
