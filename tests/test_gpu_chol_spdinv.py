"""GPU tests of the form of chol_inv_tiles that leaves A^-1 = L^-T L^-1 beside L^-1, through the
stand-alone entry clrsdp_chol_spdinv (solver.chol_spdinv), which runs one launch of it.

Bound (derived, not measured): with X the L^-1 the same call returned, every entry of A^-1 is a
length-n fp64 dot product of two columns of X, accumulated by fused MFMA steps (one rounding
each) in some order, so |G - X^T X| <= gamma_n |X|^T |X| componentwise; (n + 2) 2^-53 covers
gamma_n for n <= 128 and the 2^-64 rounding of the extended-precision reference products.

Inputs: potrf_cases kind 0 (well conditioned) and kind 1 (the same block scaled by
D = diag(2^-(i mod 40)): graded over more than 2^20 once n > 20)."""
import functools

import numpy as np
import pytest

import potrf_cases as pc

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 112, 113, 127, 128]
MIXED = [128, 17, 64, 1, 127, 33]
SENT = -7.25          # what the output buffers hold before the launch


@functools.lru_cache(maxsize=None)
def _block(n, kind, seed=11):
    from clrsdp_amd import instance as inst
    a = pc.spd_limbs(inst, n, 1, kind, seed)[0].copy()
    a.setflags(write=False)
    return a


def _check_inverse(G, X, n, what):
    """the bound of the module docstring, and exact symmetry"""
    Xl = np.tril(X).astype(np.longdouble)
    E = Xl.T @ Xl
    M = np.abs(Xl).T @ np.abs(Xl)
    bound = (n + 2) * np.longdouble(2.0) ** -53 * M
    err = np.abs(G.astype(np.longdouble) - E)
    ratio = float(np.max(err / np.where(bound > 0, bound, 1)))
    print(what, "max |G - X^T X| / bound =", ratio)
    assert np.all(err <= bound), (what, ratio)
    assert np.array_equal(G, G.T), what


@pytest.mark.parametrize("kind", [0, 1], ids=["well-conditioned", "graded"])
def test_sizes(pk, kind):
    """every size alone: A^-1 within the bound of the L^-1 of the same call and bitwise symmetric;
    L^-1 and info bitwise those of a call that asks for no A^-1, and of clrsdp_potrf"""
    for n in SIZES:
        A = _block(n, kind)
        Li, Gi, info = pk.chol_spdinv([A], fill=SENT)
        Lp, Gp, infop = pk.chol_spdinv([A], want=[False], fill=SENT)
        assert info.tolist() == [0] and infop.tolist() == [0], (n, info, infop)
        assert np.array_equal(Li[0], Lp[0]), n
        assert np.all(Gp[0] == SENT), n
        ref, iref = pk.potrf([A], inverse=True, raw_limbs=True)
        assert iref.tolist() == [0] and np.array_equal(Li[0], ref[0][0]), n
        assert np.all(np.isfinite(Gi[0])) and not np.any(Gi[0] == SENT), n
        _check_inverse(Gi[0], Li[0], n, f"n={n} kind={kind}")


def _mixed(pk, kind):
    blocks = [_block(n, kind, seed=20 + q) for q, n in enumerate(MIXED)]
    alone = [pk.chol_spdinv([a], fill=SENT) for a in blocks]
    return blocks, alone


@pytest.mark.parametrize("kind", [0, 1], ids=["well-conditioned", "graded"])
@pytest.mark.parametrize("first", [0, 1], ids=["even-blocks", "odd-blocks"])
def test_mixed_batch_alternating(pk, kind, first):
    """six sizes in one launch, A^-1 asked for on every other block: each equals, bitwise, that
    block launched alone, L^-1 likewise; the other blocks' A^-1 buffers keep the sentinel"""
    blocks, alone = _mixed(pk, kind)
    want = [(q % 2) == first for q in range(len(blocks))]
    Li, Gi, info = pk.chol_spdinv(blocks, want=want, fill=SENT)
    assert info.tolist() == [0] * len(blocks)
    for q, n in enumerate(MIXED):
        L1, G1, i1 = alone[q]
        assert np.array_equal(Li[q], L1[0]), (q, n)
        if want[q]:
            assert np.array_equal(Gi[q], G1[0]), (q, n)
            _check_inverse(Gi[q], Li[q], n, f"mixed block {q} n={n}")
        else:
            assert np.all(Gi[q] == SENT), (q, n)


@pytest.mark.parametrize("n, p", [(128, 3), (128, 70), (128, 125), (48, 20), (33, 32)],
                         ids=["tile0", "middle", "last", "n48-middle", "n33-last"])
def test_failed_block_between_good_ones(pk, n, p):
    """a block whose pivot p is negative: info as clrsdp_potrf reports it, its A^-1 untouched, the
    neighbours complete, and the call returns"""
    good0, good1 = _block(n, 0, seed=31), _block(max(n - 7, 1), 1, seed=32)
    bad = _block(n, 0, seed=33).copy()
    bad[p, p] = -1.0
    _, iref = pk.potrf([bad], inverse=True, raw_limbs=True)
    assert iref.tolist() == [16 * (p // 16) + 1]
    Li, Gi, info = pk.chol_spdinv([good0, bad, good1], fill=SENT)
    assert info.tolist() == [0, int(iref[0]), 0]
    assert np.all(Gi[1] == SENT)
    for q, a in ((0, good0), (2, good1)):
        _check_inverse(Gi[q], Li[q], a.shape[0], f"beside a failed block, block {q}")


@pytest.mark.parametrize("n, ld", [(17, 20), (64, 65), (100, 128), (128, 160), (1, 3)])
def test_pitch_larger_than_n(pk, n, ld):
    """rows n .. ld-1 of both outputs keep the sentinel; the n x n parts are those of pitch n"""
    A = _block(n, 1)
    Li, Gi, info = pk.chol_spdinv([A, A], pitch=[ld, n], fill=SENT)
    assert info.tolist() == [0, 0]
    assert Li[0].shape == (ld, n) and Gi[0].shape == (ld, n)
    assert np.all(Li[0][n:] == SENT) and np.all(Gi[0][n:] == SENT)
    assert np.array_equal(Li[0][:n], Li[1]) and np.array_equal(Gi[0][:n], Gi[1])
    _check_inverse(Gi[0][:n], Li[0][:n], n, f"n={n} pitch={ld}")
