"""GPU tests of the solver past the on-chip panel of trsm_batched (fp64 n > 1199, double-double
n > 559, quad-double n > 239): the triangular solves with the factors of S_j, Q and X then run
as the blocked chain across workgroups (TrsmPlan in csrc/clrsdp.hip: trsm_batched per super-block
and trsm_blk_update), on the LU path and on the default Cholesky path alike.

Shapes: synth(seed=3, J=2, L=1, rank=1, n_y=8, delta, N) as tests/test_gpu_lu_large.py, dim_S = N
the first multiple of 16 past each bound with dim_S <= delta (delta + 1) / 2; kappa_2(S_j) is 225 /
170 (quad-double 256), 1.08e3 / 979 (double-double 576), 649 / 633 (fp64 1216) and 19.5 / 20.5 for
the quad-double shape with X blocks of 256 (kappa_2(X) ~ 42), so the fp64 oracle is a reference
at the project's stage tolerance of 1e-11.  LU against Cholesky at fp64 1e-11, dd 1e-25, qd 1e-50.
"""
import mpmath
import numpy as np
import pytest

import test_gpu_lu_large as LL
from helpers import rel_err

pytestmark = pytest.mark.gpu

SHAPES = {4: dict(delta=32, N=256), 2: dict(delta=40, N=576), 1: dict(delta=64, N=1216)}
XSHAPE = dict(delta=256, N=300)     # quad-double X blocks of 256 > 239, dim_S = 300
TOL = LL.TOL
IDS = ["qd-256", "dd-576", "fp64-1216"]
_cache = {}


def _case(pk, oracle, words):
    return LL._case(pk, oracle, words, **SHAPES[words])


def _direction(pk, c, flags, words):
    """Q, d and the predictor direction from the device buffers (exact limb sums at words > 1)"""
    from clrsdp_amd import _lib as L
    key = (words, flags)
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


@pytest.mark.parametrize("words", [4, 2, 1], ids=IDS)
def test_lu_stage_parity_past_the_solve_panel(pk, oracle, words):
    from clrsdp_amd import _lib as L
    LL._lu_stage_compare(pk, _case(pk, oracle, words), L.FACT_LU_SQ, words)


@pytest.mark.parametrize("words", [4, 2, 1], ids=IDS)
def test_cholesky_stage_parity_past_the_solve_panel(pk, oracle, words):
    """the default flags: potrf's L through the chain (mode 0)"""
    from clrsdp_amd import _lib as L
    LL._lu_stage_compare(pk, _case(pk, oracle, words), L.FACT_FALLBACK, words)


@pytest.mark.parametrize("lu", [True, False], ids=["lu", "cholesky"])
def test_x_blocks_past_the_solve_panel(pk, oracle, lu):
    """quad-double X / Y blocks of 256: X^-1 by approx_inv! (two chained solves per block) with
    LU for S_j and Q, and the default Cholesky path of the same shape"""
    from clrsdp_amd import _lib as L
    c = LL._case(pk, oracle, 4, **XSHAPE)
    LL._lu_stage_compare(pk, c, (L.FACT_LU_SQ | L.FACT_LU_X) if lu else L.FACT_FALLBACK, 4)


@pytest.mark.parametrize("words", [4, 2, 1], ids=IDS)
def test_lu_agrees_with_cholesky_past_the_solve_panel(pk, oracle, words):
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


@pytest.mark.parametrize("words", [4, 2], ids=IDS[:2])
def test_exact_dual_newton_identity_past_the_solve_panel(pk, oracle, words):
    """Tr(A_* dY) + B dy = d from the exact device buffers, in mpmath at 320 bits, to the stage
    tolerance relative to max|c| (it holds only as far as the chained solves with the LU of S_j
    solved the Schur system at the word's precision)."""
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


def test_iterate_falls_back_to_lu_past_the_solve_panel(pk, oracle):
    """Quad-double dim_S = 256, default flags, a state whose S_j Cholesky fails: the body is
    re-run with LU (the flags gain CLRSDP_FACT_LU_SQ) and ends at the step length's cho!(Y) of
    the indefinite Y; nothing was applied."""
    from clrsdp_amd import _lib as L
    c = _case(pk, oracle, 4)
    st = LL._indefinite_Y_state(oracle, c)
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


def test_trsm_blk_0_restores_the_size_error(pk, oracle, monkeypatch):
    """CLRSDP_TRSM_BLK=0 (read when a plan is finalised): set_factorization past the panel of the
    LU triangular solves is E_ARG again.  The handle is created first: its Cholesky plans at this
    size would refuse too."""
    from clrsdp_amd import _lib as L
    c = _case(pk, oracle, 4)
    dev = pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=4)
    try:
        monkeypatch.setenv("CLRSDP_TRSM_BLK", "0")
        with pytest.raises(L.ClrsdpError) as ei:
            dev.set_factorization(L.FACT_LU_SQ)
        assert ei.value.code == L.E_ARG
        assert dev.factorization == L.FACT_FALLBACK
    finally:
        dev.close()
    with pytest.raises(L.ClrsdpError) as ei:
        pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=4)
    assert ei.value.code == L.E_ARG


def test_chain_replays_in_the_loop_body_graph(pk, oracle):
    """Two iterations at quad-double 256 with the default hipGraph replay of the loop body and the
    same two enqueued eagerly: bitwise the same states, so the chain's host loop is capture-safe."""
    c = _case(pk, oracle, 4)
    P = pk.make_params("0.3", "0.1", "0.7", 0)
    out = []
    for graph in (True, False):
        dev = pk.DeviceSolver(c["cons"], c["b"], pk.get_block_info(c["cons"]), precision_words=4)
        try:
            if not graph:
                dev.set_graph(False)
            dev.set_state(*c["state"])
            for _ in range(2):
                dev.iterate(P, False)
            out.append(dev.get_state(exact=True))
        finally:
            dev.close()
    (x0, X0, y0, Y0), (x1, X1, y1, Y1) = out
    assert np.array_equal(x0, x1) and np.array_equal(y0, y1)
    for j in range(len(X0)):
        for l in range(len(X0[j])):
            assert np.array_equal(X0[j][l], X1[j][l]) and np.array_equal(Y0[j][l], Y1[j][l])
