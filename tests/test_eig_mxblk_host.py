"""solver.eigmin_kernel with CLRSDP_EIG_MX_BLK (a host-only query: no device, no launch): the
mxblk route (CLRSDP_EIG_K_MXBLK, 6) stands exactly where the table of test_eig_dispatch_host.py
has eigmin_batched for double-double and quad-double, from the first size of that range, and
nowhere else; unset, 0 and CLRSDP_EIG_MX=0 give the table without it; CLRSDP_EIG_BLK=1 does not
move it; fp64 never takes it.

Every query reads the environment afresh, CLRSDP_EIG_MX included: with CLRSDP_EIG_MX=0 the table
with CLRSDP_EIG_MX_BLK=1 is the table with the switch unset."""
import pytest

import test_eig_dispatch_host as dh

SPLIT, MX, LDS2, LDS, BATCHED, BLK, MXBLK = range(7)   # CLRSDP_EIG_K_* (include/clrsdp.h)
# the first size the route takes, per word width (MatPlan<T>::MXBLK_NMIN): the first of
# eigmin_batched's range
NMIN = {2: 97, 4: 67}


def _table(pk):
    return {k: pk.eigmin_kernel(k[1], k[0]) for k in dh.TABLE}


def _want(chain):
    out = {}
    for (words, n), v in dh.TABLE.items():
        if v == BATCHED:
            v = MXBLK if words > 1 and n >= NMIN[words] else (BLK if chain else BATCHED)
        out[(words, n)] = v
    return out


@pytest.fixture
def env(monkeypatch):
    for name in ("CLRSDP_EIG_MX", "CLRSDP_EIG_BLK", "CLRSDP_EIG_MX_BLK"):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_route_stands_where_eigmin_batched_stood(pk, env):
    from clrsdp_amd import _lib
    assert _lib.EIG_K_MXBLK == MXBLK
    env.setenv("CLRSDP_EIG_MX_BLK", "1")
    assert _table(pk) == _want(False)
    assert MXBLK in _table(pk).values()
    for words in (2, 4):
        for nmax in range(1, 300):
            env.setenv("CLRSDP_EIG_MX_BLK", "1")
            on = pk.eigmin_kernel(nmax, words)
            env.delenv("CLRSDP_EIG_MX_BLK")
            off = pk.eigmin_kernel(nmax, words)
            want = MXBLK if off == BATCHED and nmax >= NMIN[words] else off
            assert on == want, (words, nmax, on, off)
        assert pk.eigmin_kernel(NMIN[words], words) == BATCHED


@pytest.mark.parametrize("value", [None, "0"])
def test_table_with_the_switch_off(pk, env, value):
    if value is not None:
        env.setenv("CLRSDP_EIG_MX_BLK", value)
    assert _table(pk) == dh.TABLE


def test_chain_switch_does_not_move_it(pk, env):
    env.setenv("CLRSDP_EIG_MX_BLK", "1")
    env.setenv("CLRSDP_EIG_BLK", "1")
    assert _table(pk) == _want(True)
    for words in (2, 4):
        for nmax in (NMIN[words], 160, 1024, 4096):
            assert pk.eigmin_kernel(nmax, words) == MXBLK


def test_fp64_never_takes_it(pk, env):
    env.setenv("CLRSDP_EIG_MX_BLK", "1")
    for chain in (None, "1"):
        if chain:
            env.setenv("CLRSDP_EIG_BLK", chain)
        assert all(pk.eigmin_kernel(n, 1) != MXBLK for n in list(range(1, 300)) + [1024, 4096])


def test_off_with_eig_mx_0(pk, env):
    """CLRSDP_EIG_MX=0 switches every refined-eigenpair route off: the table with
    CLRSDP_EIG_MX_BLK=1 is the table without it (eigmin_lds2 in eigmin_mx's range, eigmin_batched
    in its own)."""
    env.setenv("CLRSDP_EIG_MX", "0")
    off = _table(pk)
    env.setenv("CLRSDP_EIG_MX_BLK", "1")
    on = _table(pk)
    assert on == off
    assert MXBLK not in on.values() and MX not in on.values()
    assert on[(2, 97)] == BATCHED and on[(4, 67)] == BATCHED and on[(2, 64)] == LDS2


def test_eig_mx_0_after_an_earlier_query(pk, env):
    """Every query reads the environment afresh: CLRSDP_EIG_MX=0 takes effect after multi-word
    queries under the default in the same process, and unsetting it restores the default."""
    assert pk.eigmin_kernel(64, 2) == MX and pk.eigmin_kernel(32, 4) == MX
    env.setenv("CLRSDP_EIG_MX_BLK", "1")
    assert pk.eigmin_kernel(97, 2) == MXBLK
    env.setenv("CLRSDP_EIG_MX", "0")
    assert pk.eigmin_kernel(64, 2) == LDS2 and pk.eigmin_kernel(32, 4) == LDS2
    assert pk.eigmin_kernel(97, 2) == BATCHED
    env.delenv("CLRSDP_EIG_MX")
    assert pk.eigmin_kernel(64, 2) == MX and pk.eigmin_kernel(32, 4) == MX
    assert pk.eigmin_kernel(97, 2) == MXBLK
