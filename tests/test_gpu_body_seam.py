"""GPU tests of the seam between two fp64 loop bodies at one rank (DESIGN.md sections 6 and 7):
the synchronous body publishes its stat block into the pinned host mirror from its last scalar
launch and clrsdp_iterate polls a sequence word (no copy node, no stream sync), and chol(Q) stays
on the main stream while p, the guarded copy and the head of the predictor's solve run on the side
stream.  Neither changes a kernel's arithmetic, so everything here is bitwise: the loop body
against the ten stages run one by one (clrsdp_run_stage keeps the copy + sync and the old
threading), with both captured graphs (pd_feas 0 and 1), with the two switches off, with the
eager body of a failed capture, across set_state / save_state / restore_state, under timing
mode 2, and around a body whose factorisation fails.

The instance is the smallest that takes the fp64 strip chains (block size 65 > 64) with a
2x2-blocked S_j (dim_S = 129 > 128) on the fused Schur path:
synth(J=2, delta=65, rank=1, n_y=4)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = dict(J=2, delta=65, rank=1, n_y=4)
ROW = ("mu", "P_err", "p_err", "d_err", "alpha_p", "alpha_d", "beta_c", "p_obj", "d_obj")
# the scalar slots behind the nine fields of a log row (read_stats)
ROW_SC = ("mu", "err_P", "err_p", "err_d", "alpha_p", "alpha_d", "beta_c", "p_obj", "d_obj")
_cache = {}


def _instance(pk):
    if "inst" not in _cache:
        cons, b = pk.synth(seed=5, **CFG)
        bi = pk.get_block_info(cons)
        _cache["inst"] = (cons, b, bi, pk.make_params("0.3", "0.1", "0.7", 0),
                          pk.initial_point(bi, 10.0, 10.0))
    return _cache["inst"]


def _flat(state):
    x, X, y, Y = state
    return np.concatenate([np.ravel(x), np.ravel(y)] + [np.ravel(m) for bj in X + Y for m in bj])


def _row(st):
    return tuple(getattr(st, f) for f in ROW)


def _staged(pk, pd_feas):
    """three bodies as ten clrsdp_run_stage calls each: the log row (from the scalar slots), the
    iterate and the scalar slots after every body; computed once per pd_feas"""
    key = ("staged", pd_feas)
    if key not in _cache:
        from clrsdp_amd import _lib as L
        cons, b, bi, P, st0 = _instance(pk)
        dev = pk.DeviceSolver(cons, b, bi)
        try:
            info = dev.schur_info()
            dev.set_state(*st0)
            out = []
            for _ in range(3):
                for s in range(L.NUM_STAGES):
                    dev.run_stage(s, P, pd_feas)
                sc = dev.buffer(L.BUF_SCALARS)
                out.append((tuple(float(sc[L.SC[n]]) for n in ROW_SC), _flat(dev.get_state()), sc))
        finally:
            dev.close()
        for row, fl, sc in out:
            fl.setflags(write=False)
            sc.setflags(write=False)
        _cache[key] = (info, out)
    return _cache[key]


def _bodies(pk, dev, pd_feas, n=3):
    from clrsdp_amd import _lib as L
    out = []
    for _ in range(n):
        st = dev.iterate(_instance(pk)[3], pd_feas)
        assert st.status == 0
        out.append((_row(st), _flat(dev.get_state()), dev.buffer(L.BUF_SCALARS)))
    return out


def _assert_same(got, want):
    for k, ((r, f, s), (r0, f0, s0)) in enumerate(zip(got, want)):
        assert r == r0, (k, [(n, a, c) for n, a, c in zip(ROW, r, r0) if a != c])
        assert np.array_equal(f, f0), k
        assert np.array_equal(s, s0, equal_nan=True), (k, np.flatnonzero(s != s0))


def test_instance_takes_the_chain_path(pk):
    cons, b, bi, P, st0 = _instance(pk)
    info, _ = _staged(pk, False)
    assert bi.Y_blocksizes[0][0] > 64                # the strip chains' threshold (64 < n <= 128)
    assert 128 < min(bi.dim_S) <= 256                # S_j is factorised as 2x2 blocks
    assert info["fast"] == 1 and info["fused"] == 1, info


@pytest.mark.parametrize("switches", [{}, {"CLRSDP_SEAM_PUB": "0"}, {"CLRSDP_QCHOL_MAIN": "0"},
                                      {"CLRSDP_INJECT_CAPTURE_FAIL": "1"}],
                         ids=["default", "no-publish", "qchol-side", "eager-after-failed-capture"])
@pytest.mark.parametrize("pd_feas", [False, True])
def test_three_bodies_equal_the_stages(pk, monkeypatch, pd_feas, switches):
    """log rows (nine fields), x, X, y, Y and every scalar slot after each of three bodies"""
    cons, b, bi, P, st0 = _instance(pk)
    _, want = _staged(pk, pd_feas)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)
    dev = pk.DeviceSolver(cons, b, bi)
    try:
        dev.set_state(*st0)
        _assert_same(_bodies(pk, dev, pd_feas), want)
    finally:
        dev.close()


def test_alternating_graphs_and_state_changes(pk):
    """both captured graphs on one handle; set_state in between; save_state / restore_state between
    bodies replays the third body bitwise"""
    cons, b, bi, P, st0 = _instance(pk)
    want = {f: _staged(pk, f)[1] for f in (False, True)}
    dev = pk.DeviceSolver(cons, b, bi)
    try:
        for f in (False, True, False):
            dev.set_state(*st0)
            _assert_same(_bodies(pk, dev, f, 2), want[f])
            dev.save_state()
            third = _bodies(pk, dev, f, 1)
            _assert_same(third, want[f][2:])
            dev.restore_state()
            _assert_same(_bodies(pk, dev, f, 1), want[f][2:])
    finally:
        dev.close()


def test_timing_mode_2_reads_the_published_stamps(pk):
    from clrsdp_amd import _lib as L
    cons, b, bi, P, st0 = _instance(pk)
    _, want = _staged(pk, False)
    dev = pk.DeviceSolver(cons, b, bi)
    try:
        dev.set_timing(2)
        dev.set_state(*st0)
        for k in range(3):
            st = dev.iterate(P, False)
            assert 0.0 < st.phase_ms[L.STAGE_SCHUR] < 1e3, (k, st.phase_ms[L.STAGE_SCHUR])
            assert _row(st) == want[k][0]
        assert np.array_equal(_flat(dev.get_state()), want[2][1])
    finally:
        dev.close()


@pytest.mark.parametrize("fallback", [False, True])
def test_failed_body_then_clean_body(pk, fallback):
    """X not positive definite at set_state: the body reports the same status code as before
    and applies nothing; after a valid set_state the next body runs with clean status words and
    gives the first staged body"""
    from clrsdp_amd import _lib as L
    cons, b, bi, P, st0 = _instance(pk)
    _, want = _staged(pk, False)
    x, X, y, Y = st0
    Xbad = [[m.copy() for m in bj] for bj in X]
    Xbad[1][0][2, 2] = -5.0
    dev = pk.DeviceSolver(cons, b, bi)
    try:
        if not fallback:
            dev.set_factorization(0)
        dev.set_state(x, Xbad, y, Y)
        before = _flat(dev.get_state())
        with pytest.raises(L.ClrsdpError) as ei:
            dev.iterate(P, False)
        assert ei.value.code == (L.E_STEP if fallback else L.E_NOT_PD_X)
        assert np.array_equal(_flat(dev.get_state()), before)
        if not fallback:  # (with the fallback taken the handle stays on the LU plans: other kernels)
            dev.set_state(*st0)
            _assert_same(_bodies(pk, dev, False, 1), want[:1])
    finally:
        dev.close()
