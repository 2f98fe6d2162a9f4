"""GPU tests of the precision hand-off (clrsdp_handoff_state, DeviceSolver.handoff_state_to) and of
one solve across widths (solver.solve_escalating).

Instances: ``rank2_mp256_seed5`` (J = 2, delta = 3, rank 2, n_y = 3: X has 18 entries) and the
sphere-packing shape (unequal blocks, n_y = 52; X has 1021 entries, just under four workgroups of
the conversion kernel, whose grid-stride loop runs over 2 * 1021 + 68 + 52 = 2162 elements in 9
workgroups with a ragged last one).

  conversion   all 9 (source, destination) widths on both instances: the source holds random
               renormalised multi-limb numbers with non-zero trailing limbs; the destination's raw
               limbs (clrsdp_get_state planes, read after the source was destroyed) are the source
               limbs then zeros (wider), the same bits (equal), the leading limbs (narrower).
  bookkeeping  a double-double handle that has run bodies of its own (a captured graph, the flags
               of a finished body) and then receives a state continues bitwise like a fresh
               handle given that state by set_state.
  refusals     each case's code; nothing copied.  A failed body leaves its handle's state as it
               was set (the device guards the update), and that state can be handed over.
  escalation   fp64 -> dd at thresholds 1e-20 and fp64 -> dd -> qd at 1e-40 arrive at the 256-bit
               oracle's objectives (both runs hold gap < thr, so the objectives differ by at most
               2 thr max(1, |p + d|) each way: tolerance 4 thr max(1, |p + d|)) with fewer bodies
               at the wide width than that width alone needs; solverank1sdp is unchanged.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
WIDTHS = (1, 2, 4)
_cache = {}


def _golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def _instance(pk, name):
    if name not in _cache:
        if name == "sphere":
            cons, b = pk.synth_mixed(**pk.SPHERE_PACKING_SHAPE, seed=1)
        elif name == "c1":
            cons, b = pk.synth(J=2, delta=4, rank=1, n_y=4, seed=3)
        else:
            cons, b = pk.synth(J=2, delta=3, rank=2, n_y=3, seed=5)
        _cache[name] = (cons, b, pk.get_block_info(cons))
    return _cache[name]


def _solver(pk, name, words):
    cons, b, bi = _instance(pk, name)
    return pk.DeviceSolver(cons, b, bi, precision_words=words)


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def raw_state(dev):
    """the limbs of x, X, y, Y as the device holds them: arrays (words, n)"""
    w = dev.w
    out = [np.full(w * n, np.nan) for n in (dev.n_x, dev.n_blk, dev.bi.n_y, dev.n_blk)]
    dev.check(dev.L.clrsdp_get_state(dev.h, *[_ptr(a) for a in out]))
    return [a.reshape(w, -1) for a in out]


def set_raw_state(dev, planes):
    flat = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1) for p in planes]
    dev.check(dev.L.clrsdp_set_state(dev.h, *[_ptr(a) for a in flat]))


def random_limbs(n, words, rng):
    """renormalised numbers: limb q + 1 is below half a unit in the last place of limb q (a factor
    2^-55 .. 2^-54 smaller), never zero, signs mixed: set_state keeps them bit for bit"""
    out = np.zeros((words, n))
    out[0] = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    for q in range(1, words):
        out[q] = np.abs(out[q - 1]) * 2.0 ** -55 * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def expected_planes(src, wd):
    ws = src.shape[0]
    out = np.zeros((wd, src.shape[1]))
    out[:min(ws, wd)] = src[:min(ws, wd)]
    return out


# ---- 1. conversion ------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", WIDTHS)
@pytest.mark.parametrize("ws", WIDTHS)
@pytest.mark.parametrize("name", ["rank2", "sphere"])
def test_conversion(pk, name, ws, wd):
    src, dst = _solver(pk, name, ws), _solver(pk, name, wd)
    try:
        rng = np.random.default_rng(100 * ws + wd)
        planes = [random_limbs(n, ws, rng) for n in (src.n_x, src.n_blk, src.bi.n_y, src.n_blk)]
        if name == "sphere":
            assert src.n_blk == 1021
        set_raw_state(src, planes)
        for got, want in zip(raw_state(src), planes):   # (the source holds what the test means)
            assert same_bits(got, want)
        # the destination starts from something else entirely
        set_raw_state(dst, [np.full((wd, p.shape[1]), 7.0) * (np.arange(wd)[:, None] == 0) for p in planes])
        src.handoff_state_to(dst)
        src.close()
        for nm, got, p in zip("xXyY", raw_state(dst), planes):
            assert same_bits(got, expected_planes(p, wd)), (nm, ws, wd)
            if ws > 1 and wd > 1:
                assert np.all(got[1] != 0.0)
    finally:
        src.close()
        dst.close()


# ---- 2. bookkeeping -----------------------------------------------------------------------------
def test_used_handle_continues_like_a_fresh_one(pk):
    cons, b, bi = _instance(pk, "rank2")
    prm = pk.make_params("0.3", "0.1", "0.7", 0)
    start = pk.initial_point(bi, 10.0, 10.0)
    src, used, fresh = _solver(pk, "rank2", 1), _solver(pk, "rank2", 2), _solver(pk, "rank2", 2)
    try:
        src.set_state(*start)
        src.initial_residuals(prm)
        for _ in range(3):
            src.iterate(prm, False)
        state = raw_state(src)
        # the destination has a past: two bodies of its own (a captured graph, a finished body's flags)
        used.set_state(*start)
        used.initial_residuals(prm)
        for _ in range(2):
            used.iterate(prm, False)
        src.handoff_state_to(used)
        src.close()
        set_raw_state(fresh, [expected_planes(p, 2) for p in state])
        stats = []
        for dev in (used, fresh):
            for got, p in zip(raw_state(dev), state):
                assert same_bits(got, expected_planes(p, 2))
            # (initial_residuals reports mu, the steps and beta from the scalar slots of the last
            # body, which no state change resets, set_state's neither: what the state determines
            # are its objectives, gap and errors)
            s0 = dev.initial_residuals(prm)
            st = [dev.iterate(prm, False) for _ in range(2)]
            stats.append([(s0.p_obj, s0.d_obj, s0.P_err, s0.p_err, s0.d_err, tuple(s0.gap_w))] +
                         [(s.mu, s.alpha_p, s.alpha_d, s.beta_c, s.p_obj, s.d_obj, s.P_err, s.p_err,
                           s.d_err, tuple(s.gap_w)) for s in st])
        assert stats[0] == stats[1]
        for nm, a, c in zip("xXyY", raw_state(used), raw_state(fresh)):
            assert same_bits(a, c), nm
        assert not same_bits(raw_state(used)[1], expected_planes(state[1], 2))   # (the bodies moved it)
    finally:
        for dev in (src, used, fresh):
            dev.close()


# ---- 3. refusals --------------------------------------------------------------------------------
def _refused(pk, src, dst, code):
    with pytest.raises(pk._lib.ClrsdpError) as e:
        src.handoff_state_to(dst)
    assert e.value.code == code, (e.value.code, str(e.value))
    assert "handoff_state" in str(e.value)


def test_refusals_copy_nothing(pk):
    L = pk._lib
    prm = pk.make_params("0.3", "0.1", "0.7", 0)
    a1, a2, other, unset = (_solver(pk, "rank2", 1), _solver(pk, "rank2", 2), _solver(pk, "c1", 2),
                            _solver(pk, "rank2", 1))
    try:
        _, _, bi = _instance(pk, "rank2")
        a1.set_state(*pk.initial_point(bi, 10.0, 10.0))
        a2.set_state(*pk.initial_point(bi, 3.0, 5.0))
        other.set_state(*pk.initial_point(_instance(pk, "c1")[2], 2.0, 2.0))
        s1, s2, so = raw_state(a1), raw_state(a2), raw_state(other)

        def untouched():
            return all(same_bits(g, w) for dev, ref in ((a1, s1), (a2, s2), (other, so))
                       for g, w in zip(raw_state(dev), ref))
        assert L.lib().clrsdp_handoff_state(None, a1.h) == L.E_ARG
        assert L.lib().clrsdp_handoff_state(a1.h, None) == L.E_ARG
        _refused(pk, a1, other, L.E_ARG)      # another description
        _refused(pk, other, a2, L.E_ARG)
        _refused(pk, a1, a1, L.E_ARG)         # the same handle
        _refused(pk, unset, a2, L.E_STATE)    # a source that never had a state
        assert untouched()
        # a loop body in flight, on either side
        a1.set_control(pk.solver.make_control("1e-10", "1e-10", "1e-10"))
        a1.initial_residuals(prm)
        a1.iterate_async(prm)
        _refused(pk, a1, a2, L.E_STATE)
        _refused(pk, a2, a1, L.E_STATE)
        assert all(same_bits(g, w) for g, w in zip(raw_state(a2), s2))
        _, ran = a1.iterate_wait()
        assert ran
        moved = raw_state(a1)
        assert not same_bits(moved[1], s1[1])
        # with nothing in flight the same pair goes through
        a1.handoff_state_to(a2)
        for g, p in zip(raw_state(a2), moved):
            assert same_bits(g, expected_planes(p, 2))
    finally:
        for dev in (a1, a2, other, unset):
            dev.close()


def test_failed_body_leaves_the_state_to_hand_over(pk):
    """An fp64 handle whose Y has an indefinite block: the body fails (after the handle's own LU
    fallback), the state is bitwise what was set, and a hand-off from it succeeds."""
    _, _, bi = _instance(pk, "rank2")
    prm = pk.make_params("0.3", "0.1", "0.7", 0)
    src, dst = _solver(pk, "rank2", 1), _solver(pk, "rank2", 2)
    try:
        x, X, y, Y = pk.initial_point(bi, 10.0, 10.0)
        Y[1][0] = Y[1][0].copy()
        Y[1][0][0, 0] = -3.0
        src.set_state(x, X, y, Y)
        before = raw_state(src)
        src.initial_residuals(prm)
        with pytest.raises(pk._lib.ClrsdpError) as e:
            src.iterate(prm, False)
        assert e.value.code in pk.solver.STAGE_FAIL_CODES, e.value.code
        for nm, g, w in zip("xXyY", raw_state(src), before):
            assert same_bits(g, w), nm
        src.handoff_state_to(dst)
        src.close()
        for g, w in zip(raw_state(dst), before):
            assert same_bits(g, expected_planes(w, 2))
    finally:
        src.close()
        dst.close()


# ---- 4. / 5. one solve across widths ------------------------------------------------------------
def _check_against(res, g, thr):
    import mpmath
    mpmath.mp.prec = 320
    info = res[-1]
    assert info.status == "terminated"
    assert mpmath.mpf(res[7]) < mpmath.mpf(thr)
    p, d = mpmath.mpf(g["final"]["p_obj"]), mpmath.mpf(g["final"]["d_obj"])
    tol = 4 * mpmath.mpf(thr) * max(1, abs(p + d))
    print("objective deviations", float(abs(mpmath.mpf(res[8]) - p)), float(abs(mpmath.mpf(res[9]) - d)),
          "tolerance", float(tol), "stages", info.stages)
    assert abs(mpmath.mpf(res[8]) - p) <= tol
    assert abs(mpmath.mpf(res[9]) - d) <= tol
    assert sum(s[2] for s in info.stages) == info.iterations == len(info.log)
    assert [r[0] for r in info.log] == list(range(1, info.iterations + 1))


def test_two_widths_reach_the_dd_golden(pk):
    g = _golden("rank2_mp256_seed5_gap20")
    cons, b, bi = _instance(pk, "rank2")
    res = pk.solve_escalating(cons, b, bi, widths=(1, 2), maxiterations=g["iterations"],
                              verbose=False, return_info=True, **g["params"])
    info = res[-1]
    _check_against(res, g, "1e-20")
    assert len(info.stages) == 2
    assert info.stages[0][0] == 1 and info.stages[0][2] >= 1 and info.stages[0][1] == 1
    assert info.stages[0][3] in ("floor", "stalled") or info.stages[0][3].startswith("failed:")
    assert info.stages[1][0] == 2 and info.stages[1][3] == "terminated"
    assert info.stages[1][1] == 1 + info.stages[0][2]
    assert info.stages[1][2] < len(g["log"]) == 45
    # solverank1sdp is what it was: double-double alone stops at the oracle's iteration
    plain = pk.solverank1sdp(cons, b, bi, maxiterations=g["iterations"], precision_words=2,
                             verbose=False, return_info=True, **g["params"])
    assert plain[-1].status == "terminated" and plain[-1].iterations == 45
    assert plain[-1].stages == []


def test_three_widths_reach_the_qd_golden(pk):
    g = _golden("rank2_mp256_seed5_gap40")
    assert g["status"] == "terminated" and len(g["log"]) == 83
    cons, b, bi = _instance(pk, "rank2")
    res = pk.solve_escalating(cons, b, bi, widths=(1, 2, 4), maxiterations=g["iterations"],
                              verbose=False, return_info=True, **g["params"])
    info = res[-1]
    _check_against(res, g, "1e-40")
    assert [s[0] for s in info.stages] == [1, 2, 4]
    assert all(s[2] >= 1 for s in info.stages)
    assert info.stages[2][3] == "terminated"
    assert info.stages[2][2] < len(g["log"])
