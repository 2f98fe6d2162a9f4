"""STAGE_STEP on multi-word blocks above the on-chip bound (reg_nmax: dd 64, qd 32): potrf, two
triangular solves (trsv_wave128 for n <= 128) and eigmin (dd 72: eigmin_lds2, dd 100:
eigmin_batched, qd 40: eigmin_mx with its redo, qd 72: eigmin_batched) with a block of 12
riding in the same launches.

Instances: pk.synth_mixed of two m = 1 clusters with blocks D and 12, N = dim_S = 32, n_y = 8; the
state after two fp64 oracle iterations from initial_point(10, 10) (exact in binary64); the stages
MU_R .. STEP one by one with the default flags; X, dX, Y, dY and the scalar slots read back
exactly.

Check, for (X, dX) and (Y, dY): with lambda the reported minimum (SC_MINEIG_X / _Y), rad_b the
fp64 spectral radius of L_b^-1 dM_b L_b^-T (numpy, one digit suffices) and tol the stage
tolerance (dd 1e-25, qd 1e-50), helpers.neg_pivots at 320 bits gives
    neg_pivots(dM_b - (lambda - tol rad_b) M_b) == 0 for every block and
    neg_pivots(dM_b - (lambda + tol rad_b) M_b) >= 1 for at least one block,
which brackets the true generalised lambda_min (Sylvester's law of inertia) without an
eigen-solve and from buffers read back exactly, so an error of an earlier stage can neither mask
nor fake a failure.  alpha is min(1, -gamma / lambda) formed at 320 bits from the device's own
lambda, to the same tolerance.

neg_pivots costs about 0.8 s per count at n = 100 and grows as n^3, so D = 132 (about 15 s for
its counts) is left out.
"""
import mpmath
import numpy as np
import pytest

from helpers import _sp, neg_pivots

pytestmark = pytest.mark.gpu

TOL = {2: 1e-25, 4: 1e-50}
GAMMA = "0.7"
_STATES, _RUNS = {}, {}


def _state(pk, oracle, D):
    """(cons, b, bi, state) after two fp64 oracle iterations, once per D."""
    if D not in _STATES:
        cons, b = pk.synth_mixed([_sp(1, [D], 32), _sp(1, [12], 32)], 8, seed=7)
        bi = oracle.get_block_info(cons)
        ar = oracle.Fp64()
        prm = {k: oracle._param(ar, v) for k, v in oracle.DEFAULTS.items()}
        state = oracle.initial_point(ar, bi, 10.0, 10.0)
        for _ in range(2):
            state, _ = oracle.iteration(ar, cons, bi, b, None, ar.num(0), state, False, prm)
        _STATES[D] = (cons, b, bi, state)
    return _STATES[D]


def _run(pk, oracle, words, D):
    """The device's X, dX, Y, dY (blocks) and scalars after STAGE_STEP, once per (words, D)."""
    if (words, D) not in _RUNS:
        from clrsdp_amd import _lib as L
        from clrsdp_amd import instance as inst
        cons, b, bi, state = _state(pk, oracle, D)
        P = pk.make_params("0.3", "0.1", GAMMA, 0)
        dev = pk.DeviceSolver(cons, b, pk.get_block_info(cons), precision_words=words)
        try:
            dev.set_state(*state)
            for s in range(L.STAGE_MU_R, L.STAGE_STEP + 1):
                dev.run_stage(s, P, False)
            _, X, _, Y = dev.get_state(True)
            dX = inst.flat_to_blocks(dev.buffer(L.BUF_DXMAT, True), bi)
            dY = inst.flat_to_blocks(dev.buffer(L.BUF_DYMAT, True), bi)
            sc = {k: dev.scalar(k, True) for k in ("mineig_X", "mineig_Y", "alpha_p", "alpha_d")}
        finally:
            dev.close()
        _RUNS[(words, D)] = (bi, {"X": (X, dX, sc["mineig_X"], sc["alpha_p"]),
                                  "Y": (Y, dY, sc["mineig_Y"], sc["alpha_d"])})
    return _RUNS[(words, D)]


def _rad(M, dM):
    Mf = np.array([[float(v) for v in r] for r in M])
    Df = np.array([[float(v) for v in r] for r in dM])
    Lc = np.linalg.cholesky(Mf)
    T = np.linalg.solve(Lc, np.linalg.solve(Lc, (Df + Df.T) / 2).T)
    return float(np.max(np.abs(np.linalg.eigvalsh((T + T.T) / 2))))


@pytest.mark.parametrize("side", ["X", "Y"])
@pytest.mark.parametrize("words,D", [(2, 72), (2, 100), (4, 40), (4, 72)])
def test_step_stage_large_multiword_blocks(pk, oracle, words, D, side):
    bi, run = _run(pk, oracle, words, D)
    M, dM, lam, alpha = run[side]
    tol = TOL[words]
    below, above = [], []
    with mpmath.workprec(320):
        lam = mpmath.mpf(lam)
        assert mpmath.isfinite(lam), lam
        for j in range(bi.J):
            for l in range(bi.L[j]):
                Mb = np.array(M[j][l], dtype=object)
                Db = np.array(dM[j][l], dtype=object)
                Db = (Db + Db.T) / 2
                h = mpmath.mpf(tol) * _rad(Mb, Db)
                below.append(neg_pivots(Db - (lam - h) * Mb))
                above.append(neg_pivots(Db - (lam + h) * Mb))
        gamma = mpmath.mpf(GAMMA)
        ref = mpmath.mpf(1) if lam > -gamma else -gamma / lam
        aerr = float(abs(mpmath.mpf(alpha) - ref) / ref)
    print(f"step words={words} D={D} {side}: lambda_min {float(lam):.6g}, counts below {below} above {above}, "
          f"alpha {float(ref):.6g}, alpha error / tolerance {aerr / tol:.3g}")
    assert all(c == 0 for c in below), (below, float(lam))
    assert any(c >= 1 for c in above), (above, float(lam))
    assert aerr <= tol, (float(alpha), float(ref), aerr)
