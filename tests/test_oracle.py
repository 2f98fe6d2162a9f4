"""CPU tests of the oracle (oracle/mpmp_oracle.py) against exact identities, known answers and the
committed golden vectors -- the reference ships none of its own, so this is what
anchors the restatement ("parity unpinned" w.r.t. the Julia reference itself)."""
import json
import os

import numpy as np
import pytest

from helpers import CONFIGS_SMALL, dense_A, poly_min_instance, rand_spd, rel_err

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _random_state(bi, rng):
    X = [[rand_spd(n, rng) for n in bj] for bj in bi.Y_blocksizes]
    Y = [[rand_spd(n, rng) for n in bj] for bj in bi.Y_blocksizes]
    return X, Y


@pytest.mark.parametrize("cfg", CONFIGS_SMALL)
def test_schur_equals_dense_trace_formula(pk, oracle, cfg):
    """S_ij = Tr(A_i X^-1 A_j Y) summed over blocks (what MPMP.jl:1335-1406 assembles)."""
    cons, b = pk.synth(seed=5, **cfg)
    bi = oracle.get_block_info(cons)
    rng = np.random.default_rng(0)
    X, Y = _random_state(bi, rng)
    ar = oracle.Fp64()
    Xi = oracle.xinv(ar, X)
    S, AY = oracle.compute_S_integrated(ar, cons, Xi, Y, bi)
    for j in range(bi.J):
        D = bi.dim_S[j]
        As = [dense_A(cons[j], bi, j, t) for t in range(D)]
        Sd = np.zeros((D, D))
        for a in range(D):
            for c in range(D):
                Sd[a, c] = sum(np.trace(As[a][l] @ Xi[j][l] @ As[c][l] @ Y[j][l])
                               for l in range(bi.L[j]))
        assert rel_err(S[j], Sd) < 1e-12
        assert np.allclose(S[j], S[j].T, rtol=0, atol=1e-14 * np.abs(S[j]).max())


@pytest.mark.parametrize("cfg", [CONFIGS_SMALL[0], CONFIGS_SMALL[2], CONFIGS_SMALL[1]],
                         ids=["rank1", "rank2", "m2L2"])
def test_dense_schur_helper_matches_oracle(pk, oracle, cfg):
    """helpers.schur_dense (longdouble GEMMs: the reference of the K > 4096 Schur-stage GPU tests)
    against the oracle's own compute_T_decomposition(...).S_raw and A_Y on a random SPD state, in
    the flat buffer layout of helpers.stage_reference."""
    from helpers import schur_dense
    cons, b = pk.synth(seed=5, **cfg)
    bi = oracle.get_block_info(cons)
    X, Y = _random_state(bi, np.random.default_rng(2))
    ar = oracle.Fp64()
    Xi = oracle.xinv(ar, X)
    dec, AY = oracle.compute_T_decomposition(ar, cons, Xi, Y, bi)
    S_ref = np.concatenate([s.reshape(-1, order="F") for s in dec.S_raw])
    AY_ref = np.concatenate([AY[j][l][r][s] for j in range(bi.J) for l in range(bi.L[j])
                             for r in range(bi.m[j]) for s in range(r + 1)])
    S, A_Y = schur_dense(cons, bi, Xi, Y)
    assert S.dtype == np.longdouble and S.shape == S_ref.shape and A_Y.shape == AY_ref.shape
    assert rel_err(S, S_ref) < 1e-13
    assert rel_err(A_Y, AY_ref) < 1e-13


def test_exact_schur_reference_matches_mp_oracle(pk, oracle):
    """helpers.schur_exact (exact integers, one rounding to 256 bits: the reference of the
    graded-data GPU tests) against oracle.Mp(256)'s S and A_Y at g = 0 from the same 256-bit
    X^-1.  The oracle rounds every operation at 256 bits, so the two agree to a few hundred
    units of 2^-256 of the componentwise bound, not bitwise: 2^-240 asserted."""
    from helpers import cw_err, graded_instance, schur_exact
    cons, b, st = graded_instance(pk, 12, 1, 23, 0, seed=21)
    ar = oracle.Mp(256)
    bi = oracle.get_block_info(cons)
    consm = [pk.Cluster([[[ar.asarray(v) for v in vk] for vk in Al] for Al in cl.A], ar.asarray(cl.B),
                        ar.asarray(cl.c), [[[ar.num(x) for x in hk] for hk in Hl] for Hl in cl.H])
             for cl in cons]
    Xi = oracle.xinv(ar, [[ar.asarray(st[1][0][0])]])
    Ym = [[ar.asarray(st[3][0][0])]]
    S_o, AY_o = oracle.compute_S_integrated(ar, consm, Xi, Ym, bi)
    S, AY, bS, bA = schur_exact(cons[0], Xi[0][0], st[3][0][0])
    assert cw_err(S_o[0].reshape(-1, order="F"), S, bS) <= 2.0 ** -240
    assert cw_err(AY_o[0][0][0][0], AY, bA) <= 2.0 ** -240
    # and the float64 restatement at longdouble agrees with it too (two independent routes)
    from helpers import schur_dense
    S_d, AY_d = schur_dense(cons, bi, [[np.array(Xi[0][0], dtype=float)]], st[3])
    assert cw_err(S_d.astype(float), S, bS) <= 1e-14 and cw_err(AY_d.astype(float), AY, bA) <= 1e-14


@pytest.mark.parametrize("cfg", CONFIGS_SMALL)
def test_trace_and_weighted_A_are_adjoint(pk, oracle, cfg):
    """<sum_i a_i A_i, Z> = a . Tr(A_* Z)  (MPMP.jl:1517-1584 vs 1621-1678), and both match the
    dense constraint matrices; the A_Y shortcut (1585-1618) equals trace_A(Y)."""
    cons, b = pk.synth(seed=6, **cfg)
    bi = oracle.get_block_info(cons)
    rng = np.random.default_rng(1)
    ar = oracle.Fp64()
    Z = [[(lambda M: (M + M.T) / 2)(rng.standard_normal((n, n))) for n in bj]
         for bj in bi.Y_blocksizes]
    a = rng.standard_normal(sum(bi.dim_S))
    tr = oracle.trace_A(ar, cons, Z, bi)
    W = oracle.compute_weighted_A(ar, cons, a, bi)
    lhs = sum(np.sum(W[j][l] * Z[j][l]) for j in range(bi.J) for l in range(bi.L[j]))
    assert abs(lhs - a @ tr) < 1e-11 * (1 + abs(lhs))
    for j in range(bi.J):
        for t in range(bi.dim_S[j]):
            Ad = dense_A(cons[j], bi, j, t)
            ref = sum(np.sum(Ad[l] * Z[j][l]) for l in range(bi.L[j]))
            assert abs(tr[bi.x_indices[j] + t] - ref) < 1e-12 * (1 + abs(ref))
    X, Y = _random_state(bi, rng)
    _, AY = oracle.compute_S_integrated(ar, cons, oracle.xinv(ar, X), Y, bi)
    assert rel_err(oracle.trace_A_AY(ar, cons, AY, bi), oracle.trace_A(ar, cons, Y, bi)) < 1e-13


@pytest.mark.parametrize("cfg", CONFIGS_SMALL)
def test_search_direction_solves_newton_system(pk, oracle, cfg):
    """The 3-stage block solve (MPMP.jl:1743-1776) gives B^T dx = p and
    Tr(A_* dY) + B dy = d; dX = P + sum dx_i A_i (1779-1786)."""
    cons, b = pk.synth(seed=7, **cfg)
    bi = oracle.get_block_info(cons)
    ar = oracle.Fp64()
    prm = {k: oracle._param(ar, v) for k, v in oracle.DEFAULTS.items()}
    st = oracle.initial_point(ar, bi, 10.0, 10.0)
    st, _ = oracle.iteration(ar, cons, bi, b, None, 0.0, st, False, prm)
    _, it = oracle.iteration(ar, cons, bi, b, None, 0.0, st, False, prm)
    for key in ("pred", "corr"):
        dx, dX, dy, dY = it[key]
        Bst = oracle.stack_B(cons)
        assert rel_err(Bst.T @ dx, it["p"], np.abs(b).max()) < 1e-10
        lhs = oracle.trace_A(ar, cons, dY, bi) + Bst @ dy
        assert rel_err(lhs, it["d"], np.abs(oracle.stack_c(cons)).max()) < 1e-9
        WA = oracle.compute_weighted_A(ar, cons, dx, bi)
        for j in range(bi.J):
            for l in range(bi.L[j]):
                assert rel_err(dX[j][l], WA[j][l] + it["P"][j][l]) < 1e-13


def test_known_answer_polynomial_minimum(pk, oracle):
    """max y s.t. p(x) - y is SOS: the IPM (fp64) converges to min_x p(x)."""
    cons, b, pmin = poly_min_instance(pk)
    bi = oracle.get_block_info(cons)
    res = oracle.solverank1sdp(cons, b, bi, omega_p=10.0, omega_d=10.0, maxiterations=100,
                               duality_gap_threshold=1e-10, primal_error_threshold=1e-10,
                               dual_error_threshold=1e-10)
    assert res.status == "terminated"
    assert abs(float(res.d_obj) - pmin) < 1e-8
    assert abs(float(res.p_obj) - pmin) < 1e-8


def test_known_answer_polynomial_minimum_mp(pk, oracle):
    """Same at 128 bits: the multiprecision backend reaches a far smaller gap."""
    import mpmath
    cons, b, pmin = poly_min_instance(pk)
    ar = oracle.Mp(128)
    consm = [pk.Cluster([[[ar.asarray(v) for v in vk] for vk in cl.A[0]]], ar.asarray(cl.B),
                        ar.asarray(cl.c), [[[ar.num(x) for x in hk] for hk in cl.H[0]]])
             for cl in cons]
    bi = oracle.get_block_info(consm)
    res = oracle.solverank1sdp(consm, b, bi, ar=ar, omega_p=10.0, omega_d=10.0, maxiterations=60,
                               duality_gap_threshold="1e-20", primal_error_threshold="1e-20",
                               dual_error_threshold="1e-20")
    assert res.status == "terminated"
    assert abs(float(res.d_obj) - pmin) < 1e-12


def test_mp_backend_agrees_with_fp64(pk, oracle):
    """One loop body at 200 bits vs fp64 on a well-conditioned state."""
    cons, b = pk.synth(seed=8, J=2, delta=3, rank=1, n_y=3, m=2, L=1)
    bi = oracle.get_block_info(cons)
    a64 = oracle.Fp64()
    amp = oracle.Mp(200)
    prm64 = {k: oracle._param(a64, v) for k, v in oracle.DEFAULTS.items()}
    prmmp = {k: oracle._param(amp, v) for k, v in oracle.DEFAULTS.items()}
    consm = [pk.Cluster([[[amp.asarray(v) for v in vk] for vk in Al] for Al in cl.A],
                        amp.asarray(cl.B), amp.asarray(cl.c),
                        [[[amp.num(x) for x in hk] for hk in Hl] for Hl in cl.H]) for cl in cons]
    s64 = oracle.initial_point(a64, bi, 10.0, 10.0)
    smp = oracle.initial_point(amp, bi, 10.0, 10.0)
    s64, i64 = oracle.iteration(a64, cons, bi, b, None, 0.0, s64, False, prm64)
    smp, imp = oracle.iteration(amp, consm, bi, amp.asarray(b), None, amp.num(0), smp, False, prmmp)
    assert rel_err(np.array(smp[0], dtype=float), s64[0]) < 1e-12
    assert abs(float(imp["alpha_p"]) - i64["alpha_p"]) < 1e-12
    assert abs(float(imp["mu"]) - i64["mu"]) < 1e-12 * abs(i64["mu"])


def test_block_info_and_balancer(pk, oracle):
    cons, b = pk.synth(seed=1, J=3, delta=4, rank=1, n_y=2, m=2, L=2,
                       ranks=[[1, 0, 2, 1, 1, 1, 1], [2, 2, 0, 1, 1, 1, 1]])
    bo = oracle.get_block_info(cons)
    bp = pk.get_block_info(cons)
    for f in ("J", "n_y", "m", "L", "n_samples", "Y_blocksizes", "dim_S", "ranks", "x_indices",
              "rank_sums", "nz_k", "jl_pairs"):
        assert getattr(bo, f) == getattr(bp, f), f
    assert bp.dim_S == [3 * 7] * 3
    assert bp.rank_sums[0][0] == [0, 1, 1, 3, 4, 5, 6, 7]
    assert bp.nz_k[0][1] == 0 and bp.Y_blocksizes[0] == [8, 8]
    # balancer: partition, improves the initial contiguous split (MPMP.jl:425-465)
    w = [100, 1, 1, 1, 50, 50, 2, 2]
    sets, sw = pk.distribute_weights_swapping(w, 3)
    assert sorted(i for s in sets for i in s) == list(range(len(w)))
    assert max(sw) <= max(sum(w[0:3]), sum(w[3:6]), sum(w[6:8]))
    assert sets == oracle.distribute_weights_swapping(w, 3)[0]


@pytest.mark.parametrize("name", ["c1_fp64_seed3", "m2L2_fp64_seed4", "c1_mp256_seed3"])
def test_golden_vectors(pk, oracle, name):
    """The oracle reproduces the committed golden vectors (tests/golden/make_golden.py)."""
    path = os.path.join(GOLDEN, name + ".json")
    g = json.load(open(path))
    cons, b = pk.synth(**g["instance"])
    bi = oracle.get_block_info(cons)
    ar = oracle.Fp64()
    res = oracle.solverank1sdp(cons, b, bi, ar=ar, maxiterations=g["iterations"] + 1,
                               **g["params"])
    tol = g["tolerance_fp64"]
    for row, ref in zip(res.log, g["log"]):
        for key in ("mu", "alpha_p", "alpha_d", "beta"):
            assert abs(float(getattr(row, key)) - float(ref[key])) <= tol * max(1.0, abs(float(ref[key]))), key
    assert rel_err(res.x, np.array([float(v) for v in g["x"]])) < tol


def test_sphere_packing_golden_runs_are_consistent():
    """The two 256-bit oracle runs on the real sphere-packing instance (40 iterations, and to
    termination at the reference's default thresholds) share their first 40 log rows exactly, and
    the terminated run satisfies the stopping rule (MPMP.jl:734-742): gap < 1e-15 and the final
    objectives inside the 40-iteration bracket."""
    import mpmath
    a = json.load(open(os.path.join(GOLDEN, "sp_real_d8_mp256.json")))
    f = json.load(open(os.path.join(GOLDEN, "sp_real_d8_mp256_full.json")))
    assert a["instance"] == f["instance"]
    for ra, rf in zip(a["log"], f["log"]):
        assert all(ra[k] == rf[k] for k in ("mu", "alpha_p", "alpha_d", "beta"))
    assert f["status"] == "terminated" and len(f["log"]) > len(a["log"])
    with mpmath.workprec(256):
        fin = {k: mpmath.mpf(v) for k, v in f["final"].items()}
        assert fin["gap"] < mpmath.mpf("1e-15")
        lo, hi = sorted((mpmath.mpf(a["log"][-1]["p_obj"]), mpmath.mpf(a["log"][-1]["d_obj"])))
        assert lo <= fin["p_obj"] <= hi and lo <= fin["d_obj"] <= hi


@pytest.mark.parametrize("name,bits", [("c4dd", 128), ("c4dd", 256), ("qd32", 256)])
def test_stage_fixtures_agree_with_fp64_oracle(pk, oracle, name, bits):
    """The precomputed multi-precision stage fixtures (tests/golden/make_stage_fixtures.py) are
    consistent with the fp64 oracle run on the same stored state: every sampled entry and
    sketch within fp64 round-off times the conditioning of this mid-run state."""
    import gzip
    import importlib.util
    import json
    import os

    from helpers import compare_summary, residual_scales, stage_reference
    gdir = os.path.join(os.path.dirname(__file__), "golden")
    spec = importlib.util.spec_from_file_location("make_stage_fixtures",
                                                  os.path.join(gdir, "make_stage_fixtures.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    sf = os.path.join(gdir, f"stage_{name}.npz")
    if not os.path.exists(os.path.join(gdir, f"stage_{name}_mp{bits}.json.gz")):
        pytest.skip("fixture not generated")
    cons, b = M.instance(name, sf)
    bi = oracle.get_block_info(cons)
    state = M.load_state(sf, bi)
    ar = oracle.Fp64()
    prm = {k: oracle._param(ar, v) for k, v in oracle.DEFAULTS.items()}
    nxt, it = oracle.iteration(ar, cons, bi, b, None, 0.0, state, False, prm)
    ref = stage_reference(it, nxt, bi)
    with gzip.open(os.path.join(gdir, f"stage_{name}_mp{bits}.json.gz"), "rt") as f:
        fx = json.load(f)
    assert set(fx["buffers"]) == set(ref)
    sc = residual_scales(cons, b, state[1])
    e = {k: compare_summary(ref[k], rec, sc.get(k, 0.0)) for k, rec in fx["buffers"].items()}
    assert max(e.values()) < 1e-9, e


def test_late_stage_fixture_agrees_with_fp64_oracle(pk, oracle):
    """The late double-double fixture (c4late, make_stage_fixtures.make_late) is consistent with
    the fp64 oracle started from its state rounded to float64, on the early buffers mu and R --
    a stale or mis-indexed fixture is caught without a GPU.  mu = <X, Y> / n to 1e-9; R = mu_p I
    - X Y cancels to the size of mu, so to 1e-9 kappa with kappa = the largest kappa_1 of the X
    and Y blocks recorded in the fixture (never looser than 1e-3).  The recorded iterate is
    qualified: max kappa_1(S_j) in [1e15, 1e18]."""
    import gzip
    import importlib.util

    from helpers import compare_summary
    spec = importlib.util.spec_from_file_location("make_stage_fixtures",
                                                  os.path.join(GOLDEN, "make_stage_fixtures.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    sf = os.path.join(GOLDEN, "stage_c4late.npz")
    with gzip.open(os.path.join(GOLDEN, "stage_c4late_mp256.json.gz"), "rt") as f:
        fx = json.load(f)
    assert 20 <= fx["late_iters"] <= 30 and 1e15 <= max(fx["kappa1"]["S"]) <= 1e18
    assert set(fx["ref_err_mp106"]) == set(fx["buffers"])
    cons, b = M.instance("c4late", sf)
    bi = oracle.get_block_info(cons)
    x, X, y, Y = M.load_state(sf, bi)
    f64 = lambda a: np.array(a, dtype=float)
    X64, Y64 = [[f64(B) for B in Bj] for Bj in X], [[f64(B) for B in Bj] for Bj in Y]
    ar = oracle.Fp64()
    mu = oracle.dot_blocks(ar, X64, Y64) / bi.total_dim
    R = oracle.compute_residual_R(ar, X64, Y64, oracle._param(ar, oracle.DEFAULTS["beta_infeasible"]) * mu)
    from clrsdp_amd import instance as inst
    kappa = max(fx["kappa1"]["X"] + fx["kappa1"]["Y"])
    assert compare_summary(np.array([mu]), fx["buffers"]["mu"]) < 1e-9
    assert compare_summary(inst.blocks_to_flat(R), fx["buffers"]["R"]) < min(1e-9 * kappa, 1e-3)


@pytest.mark.parametrize("name", ["kw_C_b0_mp256", "kw_needp_mp256", "kw_needd_mp256",
                                  "kw_start_mp256"])
def test_keyword_goldens_fp64_oracle(pk, oracle, name):
    """The fp64 oracle with the golden's keywords (C, b0, need_*_feasible, initial_solutions;
    MPMP.jl:599-613) reproduces the 256-bit keyword goldens' logs to fp64 round-off and stops
    at the same iteration with the same status."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    g = json.load(open(os.path.join(GOLDEN, name + ".json")))
    cons, b = pk.synth(**g["instance"])
    bi = oracle.get_block_info(cons)
    ar = oracle.Fp64()
    kw = M.keyword_args(pk, ar, bi, g["keywords"])
    res = oracle.solverank1sdp(cons, b, bi, ar=ar, maxiterations=g["iterations"] + 1,
                               **g["params"], **kw)
    assert res.status == g["status"] and len(res.log) == len(g["log"])
    for row, ref in zip(res.log, g["log"]):
        for key in ("mu", "alpha_p", "alpha_d", "beta", "p_obj", "d_obj", "gap"):
            assert abs(float(getattr(row, key)) - float(ref[key])) <= 1e-9 * max(1.0, abs(float(ref[key]))), key
