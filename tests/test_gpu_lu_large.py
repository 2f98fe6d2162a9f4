"""GPU tests of the LU path through the solver past the on-chip panel of the one-CU getrf_batched
(quad-double n > 156, double-double n > 312, fp64 n > 624): S_j is then factored by the blocked
chain across workgroups (getrf_blk_*, LuPlan in csrc/clrsdp.hip).

Shapes: synth(seed=3, J=2, L=1, rank=1, n_y=8, delta, N), dim_S = N just past each bound, with
dim_S <= delta (delta + 1) / 2 (S_j = (V^T X^-1 V) o (V^T Y V) has at most that rank) -- S_0 is
well conditioned (kappa ~ 65 / 168 / 121), so the fp64 oracle's LU is a reference to 1e-11.
Tolerances are the project's stage tolerances (fp64 1e-11, dd 1e-25, qd 1e-50, scale-aware).
"""
import mpmath
import numpy as np
import pytest

from helpers import rel_err, residual_scales, stage_device, stage_reference

pytestmark = pytest.mark.gpu

SHAPES = {4: dict(delta=32, N=160), 2: dict(delta=40, N=320), 1: dict(delta=64, N=640)}
TOL = {1: 1e-11, 2: 1e-25, 4: 1e-50}
_cache = {}


def _case(pk, oracle, words, **shape):
    """instance, the state after two fp64 oracle iterations from Omega = 10, and the oracle's next
    iteration (computed once per shape, never modified)"""
    key = ("case", words, tuple(sorted(shape.items())))
    if key not in _cache:
        cons, b = pk.synth(seed=3, J=2, L=1, rank=1, n_y=8, **(shape or SHAPES[words]))
        ar = oracle.Fp64()
        bi = oracle.get_block_info(cons)
        prm = {k: oracle._param(ar, v) for k, v in oracle.DEFAULTS.items()}
        state = oracle.initial_point(ar, bi, 10.0, 10.0)
        for _ in range(2):
            state, _ = oracle.iteration(ar, cons, bi, b, None, ar.num(0), state, False, prm)
        nxt, it = oracle.iteration(ar, cons, bi, b, None, ar.num(0), state, False, prm)
        _cache[key] = dict(cons=cons, b=b, bi=bi, state=state, nxt=nxt, it=it)
    return _cache[key]


def _lu_stage_compare(pk, c, flags, words, tol=1e-11):
    """every stage of one iteration on the device against the fp64 oracle's (LU for S_j and Q)"""
    dev = pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=words)
    try:
        dev.set_factorization(flags)
        assert dev.factorization == flags
        dev.set_state(*c["state"])
        got = stage_device(dev, False)
    finally:
        dev.close()
    ref = stage_reference(c["it"], c["nxt"], c["bi"])
    sc = residual_scales(c["cons"], c["b"], c["state"][1])
    e = {k: rel_err(got[k], ref[k], sc.get(k, 0.0)) for k in ref}
    print({k: f"{v:.1e}" for k, v in e.items()})
    bad = {k: v for k, v in e.items() if not v <= tol}
    assert not bad, f"LU stage parity failures: {bad}"


def _direction(pk, c, flags, words):
    """Q, d and the predictor direction from the device buffers (exact limb sums at words > 1)"""
    from clrsdp_amd import _lib as L
    key = ("dir", words, flags)
    if key in _cache:
        return _cache[key]
    ex = words > 1
    P = pk.make_params("0.3", "0.1", "0.7", 0)
    dev = pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=words)
    try:
        dev.set_factorization(flags)
        dev.set_state(*c["state"])
        for s in (L.STAGE_MU_R, L.STAGE_XINV, L.STAGE_SCHUR, L.STAGE_FACTOR):
            dev.run_stage(s, P, False)
        o = {"Q": dev.buffer(L.BUF_Q, ex)}
        dev.run_stage(L.STAGE_RESIDUALS, P, False)
        o["d"] = dev.buffer(L.BUF_DVEC, ex)
        dev.run_stage(L.STAGE_PREDICTOR, P, False)
        for k, bf in (("dx", L.BUF_DX), ("dy", L.BUF_DY), ("dX", L.BUF_DXMAT), ("dY", L.BUF_DYMAT)):
            o[k] = dev.buffer(bf, ex)
    finally:
        dev.close()
    _cache[key] = o
    return o


@pytest.mark.parametrize("words", [4, 2, 1], ids=["qd-160", "dd-320", "fp64-640"])
def test_lu_stage_parity_past_the_panel(pk, oracle, words):
    from clrsdp_amd import _lib as L
    _lu_stage_compare(pk, _case(pk, oracle, words), L.FACT_LU_SQ, words)


@pytest.mark.parametrize("words", [4, 2], ids=["qd-160", "dd-320"])
def test_exact_dual_newton_identity(pk, oracle, words):
    """Tr(A_* dY) + B dy = d from the exact device buffers, in mpmath at 320 bits, to the stage
    tolerance relative to max|c|: unlike B^T dx = p this identity involves the true S, so it
    holds only as far as the LU of S_j solved the Schur system at the word's precision."""
    from clrsdp_amd import _lib as L
    from clrsdp_amd import instance as inst
    c = _case(pk, oracle, words)
    g = _direction(pk, c, L.FACT_LU_SQ, words)
    prec0 = mpmath.mp.prec
    try:
        ar = oracle.Mp(320)
        cons = [pk.Cluster([[[ar.asarray(v) for v in vk] for vk in Al] for Al in cl.A],
                           ar.asarray(cl.B), ar.asarray(cl.c),
                           [[[ar.num(x) for x in hk] for hk in Hl] for Hl in cl.H]) for cl in c["cons"]]
        dY = inst.flat_to_blocks(np.asarray(g["dY"], dtype=object), c["bi"])
        lhs = oracle.trace_A(ar, cons, dY, c["bi"]) + oracle.stack_B(cons) @ np.asarray(g["dy"], dtype=object)
        cmax = max(abs(x) for x in oracle.stack_c(cons))
        err = float(max(abs(a - b) for a, b in zip(lhs, g["d"])) / cmax)
    finally:
        mpmath.mp.prec = prec0
    print(f"dual Newton identity, words={words}: {err:.3e}")
    assert err <= TOL[words]


@pytest.mark.parametrize("words", [4, 2, 1], ids=["qd-160", "dd-320", "fp64-640"])
def test_lu_agrees_with_the_default_cholesky_path(pk, oracle, words):
    """The same build and state with the default Cholesky factorisations: Q and the predictor
    direction agree with the LU path's at the stage tolerance."""
    from clrsdp_amd import _lib as L
    c = _case(pk, oracle, words)
    lu = _direction(pk, c, L.FACT_LU_SQ, words)
    ch = _direction(pk, c, 0, words)
    with mpmath.workprec(320):  # (rel_err subtracts at the context's precision)
        e = {k: rel_err(lu[k], ch[k]) for k in ("Q", "dx", "dy", "dX", "dY")}
    print({k: f"{v:.1e}" for k, v in e.items()})
    assert all(v <= TOL[words] for v in e.values()), e
    if words > 1:  # two different factorisations: equal to round-off, not bitwise
        assert any(v > 0.0 for v in e.values()), e


def _indefinite_Y_state(oracle, c):
    """The mid-run state with Y shifted to be indefinite: S_j is then indefinite (but well
    conditioned), so its Cholesky fails while pivoted LU does not."""
    x, X, y, Y = c["state"]
    Y2 = []
    for Yj in Y:
        row = []
        for Yb in Yj:
            ev = np.linalg.eigvalsh(Yb)
            row.append(Yb - (ev[0] + 0.37 * (ev[-1] - ev[0])) * np.eye(Yb.shape[0]))
        Y2.append(row)
    return x, X, y, Y2


def test_iterate_falls_back_to_lu_past_the_panel(pk, oracle):
    """Quad-double dim_S = 160 with the default flags on a state whose S_j Cholesky fails: the
    body is re-run with LU (the flags gain CLRSDP_FACT_LU_SQ) and ends where the reference ends
    too, at the step length's cho!(Y) of the indefinite Y; nothing was applied."""
    from clrsdp_amd import _lib as L
    c = _case(pk, oracle, 4)
    st = _indefinite_Y_state(oracle, c)
    dev = pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=4)
    try:
        assert dev.factorization == L.FACT_FALLBACK
        dev.set_state(*st)
        with pytest.raises(L.ClrsdpError) as ei:
            dev.iterate(pk.make_params("0.3", "0.1", "0.7", 0), False)
        assert ei.value.code == L.E_STEP
        assert dev.factorization == L.FACT_FALLBACK | L.FACT_LU_SQ
        x, X, y, Y = dev.get_state()
        assert np.array_equal(x, st[0]) and np.array_equal(y, st[2])
        for j in range(len(X)):
            assert np.array_equal(X[j][0], st[1][j][0]) and np.array_equal(Y[j][0], st[3][j][0])
    finally:
        dev.close()


def test_lu_inverse_past_the_panel(pk, oracle):
    """X^-1 by approx_inv! (CLRSDP_FACT_LU_X) of quad-double X blocks of 160 > 156, together
    with LU for S_j (dim_S = 200) and Q, against the fp64 oracle."""
    from clrsdp_amd import _lib as L
    c = _case(pk, oracle, 4, delta=160, N=200)
    _lu_stage_compare(pk, c, L.FACT_LU_SQ | L.FACT_LU_X, 4)


def test_lu_blk_0_restores_the_size_error(pk, oracle, monkeypatch):
    """CLRSDP_LU_BLK=0: getrf_batched only, so set_factorization past its panel is E_ARG and the
    fallback leaves the Cholesky error standing, as before the chain existed."""
    from clrsdp_amd import _lib as L
    monkeypatch.setenv("CLRSDP_LU_BLK", "0")
    c = _case(pk, oracle, 4)
    dev = pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=4)
    try:
        with pytest.raises(L.ClrsdpError) as ei:
            dev.set_factorization(L.FACT_LU_SQ)
        assert ei.value.code == L.E_ARG
        dev.set_state(*_indefinite_Y_state(oracle, c))
        with pytest.raises(L.ClrsdpError) as ei:
            dev.iterate(pk.make_params("0.3", "0.1", "0.7", 0), False)
        assert ei.value.code == L.E_NOT_PD_S
        assert dev.factorization == L.FACT_FALLBACK
    finally:
        dev.close()
