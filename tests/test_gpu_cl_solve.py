"""GPU tests of the fp64 cluster solve on its own (clrsdp_cl_solve, include/clrsdp.h): cl_solve_t
and cl_solve_dx through the helper pair the loop body calls under CLRSDP_CL_SOLVE=1, on batches of
clusters of 1 .. 256 rows (one to four 64-row blocks, clusters of different sizes in one grid) and
n_y from 1 to 160 (the 32-column shares of a wave, the 128-column sweep, the quarter split of
cl_solve_dx).  Operands, exact references, the composed bound and the checks are those of
tests/oper_cases.py: the exact class must give the integers in t, in every partial slab (exact
zeros for a row block past D) and in dx; the generic class stays within the bound of t carried
through W and L.  L^-1 holds NaN everywhere above its diagonal.  Each test prints its largest
error / bound.  tests/test_oper_host.py shows without a GPU that these checks reject a row 64
that is skipped, W columns >= 128 that are dropped and a u formed without t."""
import os

import numpy as np
import pytest

import oper_cases as oc
import reduce_cases as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("cls", oc.CLASSES)
@pytest.mark.parametrize("Ds", oc.CL_BATCHES, ids=lambda d: "-".join(map(str, d)))
def test_cl_solve(pk, Ds, cls):
    worst = [0.0, 0.0, 0.0]
    nrb = -(-max(Ds) // 64)
    for ny in oc.CL_NY:
        Ls, Ws, rs, dy = oc.cl_operands(Ds, ny, cls)
        t, slabs, dx = pk.cl_solve(Ls, Ws, rs, dy)
        assert slabs.shape == (len(Ds), nrb, ny)
        for c, ((refs, bnds), D) in enumerate(zip(oc.cl_eval(Ls, Ws, rs, dy), Ds)):
            for k, (name, got) in enumerate((("t", t[c]), ("slabs", slabs[c]), ("dx", dx[c]))):
                ok, fig = oc.cl_judge(cls, got, refs[k], bnds[k])
                assert ok, f"cl_solve {name} {cls} D={Ds} cluster {c} ny={ny}: error / bound {fig:.3e}"
                worst[k] = max(worst[k], fig)
            for rb in range(-(-D // 64), nrb):                       # row blocks past D: exact zeros
                assert not np.any(slabs[c, rb]) and not np.any(np.signbit(slabs[c, rb]))
    print(f"CLSOLVE D={Ds} {cls}: error / bound t {worst[0]:.3e} slabs {worst[1]:.3e} dx {worst[2]:.3e}")


def test_cl_solve_in_the_predictor_matches_the_recorded_run(pk, monkeypatch):
    """once on a handle under CLRSDP_CL_SOLVE=1 (three clusters of 199 rows: four row blocks,
    2 x 2-blocked factors): dx and dy of the PREDICTOR stage, bitwise those recorded from the
    build before direction_solves went behind launch_cl_solve_t / launch_cl_solve_dx
    (tests/golden/cl_solve_predictor.npz)"""
    from clrsdp_amd import _lib as L
    monkeypatch.setenv("CLRSDP_CL_SOLVE", "1")
    cons, b = pk.synth(seed=5, J=3, delta=100, rank=1, n_y=40)
    bi = pk.get_block_info(cons)
    dev = pk.DeviceSolver(cons, b, bi)
    try:
        dev.set_state(*pk.initial_point(bi, 10.0, 10.0))
        prm = pk.make_params("0.3", "0.1", "0.7", 0)
        dev.initial_residuals(prm)
        for s in range(L.STAGE_PREDICTOR + 1):
            dev.run_stage(s, prm, False)
        dx, dy = dev.buffer(L.BUF_DX), dev.buffer(L.BUF_DY)
    finally:
        dev.close()
    rec = np.load(os.path.join(GOLDEN, "cl_solve_predictor.npz"))
    assert rc.bitwise(dx, rec["dx"]) and rc.bitwise(dy, rec["dy"])
