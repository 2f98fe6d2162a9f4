"""Host side of the precision escalation (no GPU): the binding of clrsdp_handoff_state, the
hand-over rule ``solver.stage_decision`` on written-out gap sequences, the orchestration of
``solver.solve_escalating`` around a fake solver (its ``solver_factory`` seam), and the rule
driven by the CPU oracle (fp64, then 106 bits) against the 256-bit golden."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

# the gaps of the states an fp64 run of c1 (J = 2, delta = 4, rank 1, n_y = 4, seed 3; omega 10,
# thresholds 1e-20) produces, body 1 first (oracle/mpmp_oracle.py, Fp64()): from body 28 on the
# gap wanders between 2e-12 and 3e-10 while alpha_d is anywhere in 0.01 .. 1
C1_FP64_GAPS = [
    1.051, 1.018, 1.02, 1.059, 1.102, 0.9067, 0.4729, 0.2051, 0.08478, 0.03151, 0.01042, 0.003228,
    0.0009775, 0.0002942, 8.84e-05, 2.655e-05, 7.972e-06, 2.393e-06, 7.184e-07, 2.156e-07, 6.47e-08,
    1.941e-08, 5.825e-09, 1.748e-09, 5.244e-10, 1.573e-10, 4.722e-11, 1.544e-11, 7.586e-12,
    5.184e-12, 1.871e-11, 7.678e-12, 4.157e-12, 3.881e-12, 2.592e-10, 9.59e-11, 3.019e-11, 9.863e-12,
    4.727e-12, 3.525e-12, 2.466e-11, 8.977e-12, 5.508e-12, 9.308e-12, 5.055e-12, 6.974e-12,
    2.875e-12, 2.207e-12, 1.355e-11, 4.862e-12, 2.808e-12, 2.819e-11, 1.002e-11, 4.071e-12]


# ---- 1. the symbol --------------------------------------------------------------------------
def test_symbol_is_exported_and_bound(pk):
    L = pk._lib
    assert "clrsdp_handoff_state" in L.EXPORTS
    lib = L.lib()
    assert lib.clrsdp_handoff_state.restype is not None
    assert lib.clrsdp_handoff_state(None, None) == L.E_ARG
    assert b"null" in lib.clrsdp_last_error(None)
    assert callable(pk.DeviceSolver.handoff_state_to)
    assert pk.solve_escalating is pk.solver.solve_escalating
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "clrsdp.h")) as f:
        assert "int32_t clrsdp_handoff_state(clrsdp_handle* dst, clrsdp_handle* src);" in f.read()


# ---- 2. the rule ----------------------------------------------------------------------------
def _first_stop(pk, gaps, floor, patience):
    """the body after which stage_decision first answers, and its answer (asked on every prefix)"""
    stage_decision = pk.solver.stage_decision
    for k in range(len(gaps) + 1):
        why = stage_decision(gaps[:k], floor, patience)
        if why:
            return k, why
    return None, None


def test_floor_needs_two_states_of_this_stage(pk):
    sd = pk.solver.stage_decision
    assert sd([], 1e-8, 5) is None                     # only the state the stage started from
    assert sd([0.0], 1e-8, 5) is None                  # one state below the floor (an exact 0 too)
    assert sd([1.0, 1e-9], 1e-8, 5) is None
    assert sd([1e-9, 1.0], 1e-8, 5) is None
    assert sd([1.0, 1e-9, 1e-10], 1e-8, 5) == "floor"  # two in a row
    assert sd([1e-9, 1e-9], 1e-8, 5) == "floor"
    assert sd([1e-9, 1e-9], 0, 5) is None              # 0 and None: no floor
    assert sd([1e-9, 1e-9], None, 5) is None
    assert sd([1e-8, 1e-8], 1e-8, 5) is None           # below, not at
    # the gap of the initial point is 0 and belongs to no body: a run whose first body leaves a
    # small gap while infeasible is not handed over on it
    assert _first_stop(pk, [1e-9, 1.0, 0.5, 0.2, 0.1, 1e-9, 1e-10], 1e-8, 50) == (7, "floor")


def test_floor_at_the_width_of_the_gap(pk):
    import mpmath
    GAP_FLOORS, sd = pk.solver.GAP_FLOORS, pk.solver.stage_decision
    assert GAP_FLOORS == {1: 1e-8, 2: 1e-16}
    g = [mpmath.mpf("3e-16"), mpmath.mpf("9e-17"), mpmath.mpf("2.7e-17")]
    assert sd(g[:2], GAP_FLOORS[2], 5) is None
    assert sd(g, GAP_FLOORS[2], 5) == "floor"


def test_patience_counts_the_stage_s_own_states(pk):
    sd = pk.solver.stage_decision
    down = [2.0 ** -k for k in range(12)]
    assert _first_stop(pk, down, 0, 5) == (None, None)              # a new minimum every body
    assert sd([1.0] * 5, 0, 5) is None                          # five states: nothing to compare with
    assert sd([1.0] * 6, 0, 5) == "stalled"                     # five states after the first, none lower
    assert sd([1.0, 2.0, 2.0, 2.0, 2.0, 0.5], 0, 5) is None      # the fifth sets a new minimum
    assert sd([1.0, 2.0, 2.0, 2.0, 2.0, 1.0], 0, 5) == "stalled"  # equalling it is not a new one
    assert sd([1.0] * 6, 0, 0) is None                          # patience 0: never
    # a stage's history starts empty whatever came before it: the same five states that stall a
    # history of six do not stall on their own
    assert sd([3.0, 3.0, 3.0, 3.0, 3.0], 0, 5) is None
    assert _first_stop(pk, [1.0, 0.5] + [0.7] * 10, 0, 3) == (5, "stalled")


def test_c1_fp64_stalls_at_body_39(pk):
    assert min(C1_FP64_GAPS[:34]) == C1_FP64_GAPS[33] == 3.881e-12   # body 34: the last minimum
    assert _first_stop(pk, C1_FP64_GAPS, 0, 5) == (39, "stalled")
    # with the default fp64 floor the hand-over comes long before: bodies 23 and 24 are below 1e-8
    assert _first_stop(pk, C1_FP64_GAPS, 1e-8, 5) == (24, "floor")
    # the wandering run still sets a new minimum every few bodies (40, 47, 48): patience decides
    # how long to look
    assert _first_stop(pk, C1_FP64_GAPS, 0, 4) == (38, "stalled")
    assert _first_stop(pk, C1_FP64_GAPS, 0, 6) == (46, "stalled")


# ---- 3. the orchestration ---------------------------------------------------------------------
class FakeSolver:
    """What solve_escalating uses of a DeviceSolver.  The state is the number n of bodies applied
    to it; its objectives are 1 +- gaps(n), so the gap is gaps(n) and the errors are 0."""

    def __init__(self, pk, words, world, gaps, fail, events):
        self.pk, self.w, self.world, self.timing = pk, words, world, False
        self.gaps, self.fail, self.events = gaps, fail, events
        self.n, self.flags, self.closed = None, 1, False
        events.append(("create", words))

    def _stats(self):
        st = self.pk._lib.IterStats()
        g = self.gaps(self.n)
        st.p_obj, st.d_obj = 1.0 + g, 1.0 - g
        st.gap_w[0] = g
        st.alpha_p = st.alpha_d = 1.0
        return st

    def set_state(self, x, X, y, Y):
        self.n = 0
        self.events.append(("set_state", self.w))

    def handoff_state_to(self, other):
        self.events.append(("handoff", self.w, other.w, self.n))
        other.n = self.n

    def set_factorization(self, flags):
        self.flags = flags
        self.events.append(("set_factorization", self.w, flags))

    @property
    def factorization(self):
        return self.flags

    def set_control(self, ctl):
        pass

    def initial_residuals(self, prm):
        self.events.append(("initial_residuals", self.w, self.n))
        return self._stats()

    def iterate(self, prm, pd_feas):
        code = self.fail.get((self.w, self.n + 1))
        if code:
            self.flags |= 2   # (the handle tried its LU fallback first)
            raise self.pk._lib.ClrsdpError(code, "fake failure")
        self.n += 1
        return self._stats()

    def buffer(self, buf, exact=False):
        import mpmath
        L = self.pk._lib
        if buf == L.BUF_SCALARS:
            sc = [mpmath.mpf(0)] * 32
            g = mpmath.mpf(self.gaps(self.n))
            sc[L.SC["p_obj"]], sc[L.SC["d_obj"]] = 1 + g, 1 - g
            return sc
        return np.zeros(1)

    def get_state(self):
        return self.n, None, None, None

    def global_P_d(self):
        return None, None

    def close(self):
        if not self.closed:
            self.events.append(("close", self.w))
        self.closed = True


def _run(pk, gaps, fail=None, world=1, **kw):
    events, made = [], []

    def factory(words):
        made.append(FakeSolver(pk, words, world, gaps, fail or {}, events))
        return made[-1]
    cons, b = pk.synth(J=2, delta=3, rank=1, n_y=3, seed=1)
    args = dict(verbose=False, return_info=True, solver_factory=factory, duality_gap_threshold=1e-3)
    args.update(kw)
    try:
        return pk.solve_escalating(cons, b, pk.get_block_info(cons), **args), events, made
    except Exception as e:
        e.events, e.made = events, made
        raise


def test_failed_body_hands_over_the_state_before_it(pk):
    L = pk._lib
    res, events, made = _run(pk, lambda n: 0.5 ** n, fail={(1, 4): L.E_NOT_PD_S}, widths=(1, 2),
                             factorization=L.FACT_FALLBACK)
    info = res[-1]
    assert [e for e in events if e[0] == "handoff"] == [("handoff", 1, 2, 3)]   # once, the state before body 4
    assert ("initial_residuals", 2, 3) in events                               # where the next stage starts
    assert info.stages == [(1, 1, 3, "failed:%d" % L.E_NOT_PD_S), (2, 4, 7, "terminated")]
    assert info.stages[0][3] == "failed:4"
    assert info.status == "terminated" and info.iterations == 10 and res[0] == 10
    assert [r[0] for r in info.log] == list(range(1, 11))
    assert all(a[1] <= c[1] for a, c in zip(info.log, info.log[1:]))           # one clock
    # one handle per stage: the second is created after the first stage ended, the first closed
    # after the hand-over; each gets the caller's flags afresh (the first one's LU flag is not inherited)
    assert events.index(("create", 2)) > events.index(("initial_residuals", 1, 0))
    assert events.index(("close", 1)) == events.index(("handoff", 1, 2, 3)) + 1
    assert ("set_factorization", 2, L.FACT_FALLBACK) in events and info.factorization == L.FACT_FALLBACK
    assert all(s.closed for s in made)
    assert isinstance(res[7], __import__("mpmath").mpf)                        # the tuple of the final width


def test_other_errors_propagate(pk):
    L = pk._lib
    with pytest.raises(L.ClrsdpError) as e:
        _run(pk, lambda n: 0.5 ** n, fail={(1, 2): L.E_HIP}, widths=(1, 2))
    assert e.value.code == L.E_HIP
    assert not [ev for ev in e.value.events if ev[0] == "handoff"]
    assert all(s.closed for s in e.value.made)
    # at the last width every error is solverank1sdp's
    with pytest.raises(L.ClrsdpError) as e:
        _run(pk, lambda n: 0.5 ** n, fail={(2, 5): L.E_NOT_PD_S}, widths=(2,))
    assert e.value.code == L.E_NOT_PD_S


def test_floor_stall_and_the_iteration_bound(pk):
    res, events, _ = _run(pk, lambda n: 3 * 10.0 ** -n, widths=(1, 2, 4), duality_gap_threshold=1e-30)
    # fp64: 3e-9 and 3e-10 are the first two states below 1e-8; dd: 3e-17 and 3e-18 below 1e-16
    assert res[-1].stages == [(1, 1, 10, "floor"), (2, 11, 8, "floor"), (4, 19, 13, "terminated")]
    res, events, _ = _run(pk, lambda n: 3 * 10.0 ** -n, widths=(1, 2), gap_floors=(1e-3,),
                          duality_gap_threshold=1e-30)
    assert res[-1].stages[0] == (1, 1, 5, "floor")
    # a width whose gap stops falling: handed over after `patience` states without a new minimum
    # (bodies 8, 9 and 10 leave 1e-6, which body 7 had reached)
    res, events, _ = _run(pk, lambda n: max(3 * 10.0 ** -n, 1e-6), widths=(1, 2), patience=3,
                          maxiterations=13, duality_gap_threshold=1e-30)
    assert res[-1].stages == [(1, 1, 10, "stalled"), (2, 11, 2, "maxiterations")]
    assert res[-1].status == "maxiterations" and res[-1].iterations == 12
    # the bound counts the bodies of all stages together, and a stage it ends hands nothing over
    res, events, _ = _run(pk, lambda n: 3 * 10.0 ** -n, widths=(1, 2), maxiterations=6,
                          duality_gap_threshold=1e-30)
    assert res[-1].stages == [(1, 1, 5, "maxiterations")]
    assert not [e for e in events if e[0] == "handoff"]
    # terminate() at the caller's thresholds comes first: the solve ends at the narrow width
    res, events, _ = _run(pk, lambda n: 3 * 10.0 ** -n, widths=(1, 2), duality_gap_threshold=1e-3)
    assert res[-1].stages == [(1, 1, 4, "terminated")] and not isinstance(res[7], __import__("mpmath").mpf)


def test_arguments(pk):
    ok = lambda n: 0.5 ** n
    for kw in (dict(widths=(2, 1)), dict(widths=(1, 1)), dict(widths=(1, 3)), dict(widths=()),
               dict(precision_words=2), dict(solver=object()), dict(pipelined=True),
               dict(widths=(1, 2), gap_floors=(1e-8, 1e-16)), dict(widths=(1, 2, 4), gap_floors=(1e-8,)),
               dict(widths=(1, 2), gap_floors=(-1.0,))):
        with pytest.raises(ValueError):
            _run(pk, ok, **kw)
    with pytest.raises(ValueError):      # sharded over ranks
        _run(pk, ok, world=2, widths=(1, 2))
    assert _run(pk, ok, pipelined=False, widths=(1,))[0][-1].stages == [(1, 1, 10, "terminated")]
    import inspect
    a, e = (inspect.signature(f).parameters for f in (pk.solverank1sdp, pk.solve_escalating))
    assert set(a) <= set(e)              # every solverank1sdp keyword
    assert pk.solver.RunInfo(0, [], None, 0.0, 0.0, "terminated").stages == []


# ---- 4. the rule driven by the oracle -----------------------------------------------------------
def _oracle_stage(O, ar, cons, b, bi, state, params, stop, budget):
    """O.solverank1sdp's loop (C = 0, b0 = 0) from `state`, with solve_escalating's questions
    between two bodies; returns (state, bodies, reason, p_obj, d_obj, gap)."""
    prm = {k: O._param(ar, params.get(k, v)) for k, v in O.DEFAULTS.items()}
    thr = [prm[k] for k in ("duality_gap_threshold", "primal_error_threshold", "dual_error_threshold")]
    b, b0 = ar.asarray(b), ar.num(0)
    x, X, y, Y = state
    P, p, d = O.compute_residuals(ar, cons, x, X, y, Y, b, None, bi, use_AY=False)
    history, bodies = [], 0
    while True:
        p_obj, d_obj = O.primal_objective(ar, cons, x, b0), O.dual_objective(ar, y, Y, b, None, b0)
        gap = O.duality_gap(ar, p_obj, d_obj)
        if bodies:
            history.append(gap)
        perr, derr = max(O.max_abs_vec(ar, p), O.max_abs_blocks(ar, P)), O.max_abs_vec(ar, d)
        if O.terminate(gap, perr, derr, *thr, False, False):
            reason = "terminated"
        elif bodies >= budget:
            reason = "maxiterations"
        else:
            reason = stop(history) if stop else None
        if reason:
            return (x, X, y, Y), bodies, reason, p_obj, d_obj, gap
        pd_feas = perr < thr[1] and derr < thr[2]
        try:
            (x, X, y, Y), inter = O.iteration(ar, cons, bi, b, None, b0, (x, X, y, Y), pd_feas, prm)
        except (np.linalg.LinAlgError, ZeroDivisionError, ValueError):
            if stop is None:
                raise
            return (x, X, y, Y), bodies, "failed", p_obj, d_obj, gap
        P, p, d = inter["P"], inter["p"], inter["d"]
        bodies += 1


@pytest.mark.slow
def test_rule_on_the_oracle_reaches_the_golden(pk, oracle):
    import mpmath
    GAP_FLOORS, stage_decision = pk.solver.GAP_FLOORS, pk.solver.stage_decision
    O = oracle
    with open(os.path.join(GOLDEN, "rank2_mp256_seed5_gap20.json")) as f:
        g = json.load(f)
    assert g["status"] == "terminated" and len(g["log"]) == 45
    cons, b = pk.synth(**g["instance"])
    bi = O.get_block_info(cons)
    f64 = O.Fp64()
    state, n1, why, *_ = _oracle_stage(
        O, f64, cons, b, bi, O.initial_point(f64, bi, g["params"]["omega_p"], g["params"]["omega_d"]),
        g["params"], lambda h: stage_decision(h, GAP_FLOORS[1], 5), g["iterations"])
    assert why == "floor" and n1 >= 1, (why, n1)
    ar = O.Mp(106)
    consm = [pk.Cluster([[[ar.asarray(v) for v in vk] for vk in Al] for Al in cl.A], ar.asarray(cl.B),
                        ar.asarray(cl.c), [[[ar.num(x) for x in hk] for hk in Hl] for Hl in cl.H])
             for cl in cons]
    x, X, y, Y = state
    state = (ar.asarray(x), [[ar.asarray(m) for m in r] for r in X], ar.asarray(y),
             [[ar.asarray(m) for m in r] for r in Y])
    state, n2, why, p_obj, d_obj, gap = _oracle_stage(O, ar, consm, b, bi, state, g["params"], None,
                                                      g["iterations"] - n1)
    mpmath.mp.prec = 320
    p, d = mpmath.mpf(g["final"]["p_obj"]), mpmath.mpf(g["final"]["d_obj"])
    tol = mpmath.mpf("4e-20") * max(1, abs(p + d))
    print("fp64 bodies", n1, "106-bit bodies", n2, "gap", float(gap), "deviations",
          float(abs(p_obj - p)), float(abs(d_obj - d)), "tolerance", float(tol))
    assert why == "terminated" and gap < mpmath.mpf("1e-20")
    assert abs(p_obj - p) <= tol and abs(d_obj - d) <= tol
    assert n2 < 45, n2
