"""GPU tests of X^-1 and Q^-1 formed inside chol_inv_tiles (CLRSDP_CHOL_SPDINV, default on) in the
solver's own stages, at the smallest instance of the stage-parity tests whose X blocks reach 128
(test_gpu_parity.CONFIGS_GPU: J = 2, delta = 128, rank 1, n_y = 128, so Q is 128 x 128 as well).

XINV and chol(Q) alone: with the switch on and with =0 (the GEMMs q_xinv / q_qinv behind the
factorisation) the inverse satisfies the dot-product bound of tests/test_gpu_chol_spdinv.py against
the L^-1 of its own run, and the two L^-1 buffers are bitwise equal.  One full loop body, switch
on: the replayed graph, the eager body and the ten stages give bitwise the same iterate and log
row; against the switch off the log row agrees to test_gpu_parity's fp64 tolerance."""
import numpy as np
import pytest

from helpers import rel_err
from test_gpu_chol_spdinv import _check_inverse
from test_gpu_parity import CONFIGS_GPU, TOL64

pytestmark = pytest.mark.gpu

CFG = next(c for c in CONFIGS_GPU if c["delta"] == 128)
ROW = ("mu", "P_err", "p_err", "d_err", "alpha_p", "alpha_d", "beta_c", "p_obj", "d_obj")
ROW_SC = ("mu", "err_P", "err_p", "err_d", "alpha_p", "alpha_d", "beta_c", "p_obj", "d_obj")
_cache = {}


def _instance(pk):
    if "inst" not in _cache:
        cons, b = pk.synth(seed=3, **CFG)
        bi = pk.get_block_info(cons)
        _cache["inst"] = (cons, b, bi, pk.make_params("0.3", "0.1", "0.7", 0),
                          pk.initial_point(bi, 10.0, 10.0))
    return _cache["inst"]


def _env(monkeypatch, on):
    if on:
        monkeypatch.delenv("CLRSDP_CHOL_SPDINV", raising=False)
    else:
        monkeypatch.setenv("CLRSDP_CHOL_SPDINV", "0")


def _flat(state):
    x, X, y, Y = state
    return np.concatenate([np.ravel(x), np.ravel(y)] + [np.ravel(m) for bj in X + Y for m in bj])


def _stages(pk, monkeypatch, on):
    """one body after one warm-up body (so X is no multiple of the identity), stage by stage: the
    buffers after XINV and FACTOR, the log row and the iterate; once per switch value"""
    if ("stages", on) not in _cache:
        from clrsdp_amd import _lib as L
        cons, b, bi, P, st0 = _instance(pk)
        _env(monkeypatch, on)
        dev = pk.DeviceSolver(cons, b, bi)
        try:
            dev.set_state(*st0)
            out = {}
            for body in range(2):
                for s in range(L.NUM_STAGES):
                    dev.run_stage(s, P, False)
                    if body == 1 and s == L.STAGE_XINV:
                        out["Xinv"], out["LX"] = dev.buffer(L.BUF_XINV), dev.buffer(L.BUF_LXINV)
                    if body == 1 and s == L.STAGE_FACTOR:
                        out["Qinv"], out["LQ"] = dev.buffer(L.BUF_QINV), dev.buffer(L.BUF_LQINV)
            sc = dev.buffer(L.BUF_SCALARS)
            out["row"] = tuple(float(sc[L.SC[n]]) for n in ROW_SC)
            out["state"] = _flat(dev.get_state())
        finally:
            dev.close()
        _cache[("stages", on)] = out
    return _cache[("stages", on)]


def test_the_instance_takes_the_fused_form(pk, monkeypatch):
    cons, b, bi, P, st0 = _instance(pk)
    n = bi.Y_blocksizes[0][0]
    assert n == 128 and CFG["n_y"] <= 128
    _env(monkeypatch, True)
    assert pk.spdinv_kernel(n) and pk.spdinv_kernel(CFG["n_y"])
    _env(monkeypatch, False)
    assert not pk.spdinv_kernel(n)


def test_xinv_stage_alone(pk, monkeypatch):
    cons, b, bi, P, st0 = _instance(pk)
    on, off = _stages(pk, monkeypatch, True), _stages(pk, monkeypatch, False)
    assert np.array_equal(on["LX"], off["LX"])
    n = bi.Y_blocksizes[0][0]
    nblk = on["LX"].size // (n * n)
    assert nblk * n * n == on["LX"].size and nblk >= 2
    for name, r in (("on", on), ("off", off)):
        for q in range(nblk):
            X = r["LX"][q * n * n:(q + 1) * n * n].reshape((n, n), order="F")
            G = r["Xinv"][q * n * n:(q + 1) * n * n].reshape((n, n), order="F")
            if name == "on":
                assert np.array_equal(G, G.T), q
                _check_inverse(G, X, n, f"Xinv block {q}, switch on")
            else:   # (the GEMM's two triangles are separate dot products: the bound only)
                _check_inverse(np.tril(G) + np.tril(G, -1).T, X, n, f"Xinv block {q} lower, switch off")
                _check_inverse(np.triu(G) + np.triu(G, 1).T, X, n, f"Xinv block {q} upper, switch off")


def test_q_inverse_alone(pk, monkeypatch):
    on, off = _stages(pk, monkeypatch, True), _stages(pk, monkeypatch, False)
    n = CFG["n_y"]
    # (Q itself comes from X^-1, which differs by rounding between the two runs: each Q^-1
    # against the L_Q^-1 of its own run)
    for name, r in (("on", on), ("off", off)):
        X = r["LQ"].reshape((n, n), order="F")
        G = r["Qinv"].reshape((n, n), order="F")
        if name == "on":
            assert np.array_equal(G, G.T)
            _check_inverse(G, X, n, "Qinv, switch on")
        else:
            _check_inverse(np.tril(G) + np.tril(G, -1).T, X, n, "Qinv lower, switch off")
            _check_inverse(np.triu(G) + np.triu(G, 1).T, X, n, "Qinv upper, switch off")


def test_q_factor_bitwise_on_the_same_q(pk, monkeypatch):
    """chol(Q) of the same Q with and without Q^-1 formed beside it (the stand-alone entry on the
    Q of the staged run): L_Q^-1 bitwise equal, and it is the stage's L_Q^-1"""
    from clrsdp_amd import _lib as L
    cons, b, bi, P, st0 = _instance(pk)
    _env(monkeypatch, True)
    n = CFG["n_y"]
    dev = pk.DeviceSolver(cons, b, bi)
    try:
        dev.set_state(*st0)
        for s in range(L.STAGE_FACTOR + 1):
            dev.run_stage(s, P, False)
        Q = dev.buffer(L.BUF_Q).reshape((n, n), order="F")
        LQ = dev.buffer(L.BUF_LQINV).reshape((n, n), order="F")
        Qinv = dev.buffer(L.BUF_QINV).reshape((n, n), order="F")
    finally:
        dev.close()
    Li, Gi, info = pk.chol_spdinv([Q, Q], want=[True, False])
    assert info.tolist() == [0, 0]
    assert np.array_equal(Li[0], Li[1])
    assert np.array_equal(np.tril(LQ), Li[0]) and np.array_equal(Qinv, Gi[0])


def test_one_body_three_ways_bitwise(pk, monkeypatch):
    """switch on: the replayed graph, the eager body and the staged path; and the log row against
    the switch off"""
    cons, b, bi, P, st0 = _instance(pk)
    want = _stages(pk, monkeypatch, True)
    off = _stages(pk, monkeypatch, False)
    _env(monkeypatch, True)
    for graph in (True, False):
        dev = pk.DeviceSolver(cons, b, bi)
        try:
            dev.set_graph(graph)
            dev.set_state(*st0)
            for _ in range(2):
                st = dev.iterate(P, False)
                assert st.status == 0
            row = tuple(getattr(st, f) for f in ROW)
            assert row == want["row"], (graph, [(n, a, c) for n, a, c in zip(ROW, row, want["row"]) if a != c])
            assert np.array_equal(_flat(dev.get_state()), want["state"]), graph
        finally:
            dev.close()
    for name, a, c in zip(ROW, want["row"], off["row"]):
        e = rel_err([a], [c])
        print(name, a, c, e)
        assert e <= TOL64, (name, a, c, e)
