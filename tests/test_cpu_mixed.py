"""CPU tests of the mixed instances (helpers.MIXED) and of the per-piece metric they are compared
with: the C++ restatement (oracle/cpurest), which shares no code with the device path, against
the same references and at the same tolerances as tests/test_gpu_mixed.py.  It establishes that
the per-piece tolerances are attainable on these instances by the reference algorithm at the
device's own precisions, before the GPU tests assert them."""
import gzip
import importlib.util
import json
import os

import mpmath
import numpy as np
import pytest

from helpers import (compare_pieces, mixed_oracle_case, piecewise_err, rel_err, stage_pieces, summarize_pieces,
                     worst)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
STATE_KEYS = ("x+", "X+", "y+", "Y+")
LOG_KEYS = ("mu", "alpha_p", "alpha_d", "beta_c")   # columns 0..3 of the restatement's log


@pytest.fixture(scope="module")
def cr():
    from oracle import cpurest
    cpurest.build()
    return cpurest


@pytest.fixture(scope="module")
def fixtures():
    spec = importlib.util.spec_from_file_location("make_stage_fixtures", os.path.join(GOLDEN, "make_stage_fixtures.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return M


def _new_state(pk, cr, cons, b, bi, words, state):
    """One body of the restatement from ``state``: the stage-buffer dictionary of the new state
    and the four logged scalars."""
    from clrsdp_amd import instance as inst
    rc, log, _, (x, X, y, Y) = cr.run(pk, cons, b, bi, words, state, 1, threads=4)
    assert rc == 1, rc
    got = {"x+": np.asarray(x), "X+": inst.blocks_to_flat(X), "y+": np.asarray(y), "Y+": inst.blocks_to_flat(Y)}
    for q, k in enumerate(LOG_KEYS):
        got[k] = np.array([log[0, q]], dtype=object)
    return got


def test_stage_pieces_tile_every_buffer(pk, oracle):
    """The pieces of every key are disjoint, in order, and cover the oracle's buffer exactly, on
    an instance with m = 2, L = 2 and unequal ranks among m = 1 clusters; and the per-piece
    metric sees an error in the small cluster that the whole-buffer metric hides."""
    from helpers import stage_reference
    cons, b = pk.synth_mixed([dict(m=1, deltas=[3], N=5), dict(m=2, deltas=[4, 2], N=7, ranks=[[1, 0, 2, 1, 1, 3, 1],
                                                                                         [1, 1, 0, 2, 1, 1, 1]]),
                              dict(m=1, deltas=[6], N=11)], 4, seed=7)
    bi = oracle.get_block_info(cons)
    ar = oracle.Fp64()
    prm = {k: oracle._param(ar, v) for k, v in oracle.DEFAULTS.items()}
    st = oracle.initial_point(ar, bi, 10.0, 10.0)
    nxt, it = oracle.iteration(ar, cons, bi, b, None, ar.num(0), st, False, prm)
    ref = stage_reference(it, nxt, bi)
    pieces = stage_pieces(bi)
    assert set(pieces) == set(ref)
    for k, ps in pieces.items():
        assert ps[0][1] == 0 and ps[-1][2] == len(np.asarray(ref[k]).ravel()), k
        assert all(a[2] == c[1] and a[1] < a[2] for a, c in zip(ps, ps[1:])), k
        assert len({p[0] for p in ps}) == len(ps), k
    # S of cluster 0 is 5 x 5 at a smaller scale than cluster 2's 11 x 11 (X0 = sum A_i grows with N)
    got = {k: np.array(v, dtype=float) for k, v in ref.items()}
    a, c = pieces["Xinv"][0][1:]
    small = float(np.max(np.abs(got["Xinv"][a:c])))
    big = float(np.max(np.abs(got["Xinv"])))
    got["Xinv"][a] += 1e-9 * small
    e = piecewise_err(got, ref, bi)
    assert e[("Xinv", "j0l0")] == pytest.approx(1e-9, rel=1e-3)
    assert rel_err(got["Xinv"], ref["Xinv"]) == pytest.approx(1e-9 * small / big, rel=1e-3)
    assert all(v == 0.0 for k, v in e.items() if k != ("Xinv", "j0l0"))
    # and the fixture records: the same pieces, the same error
    recs = summarize_pieces({"Xinv": ref["Xinv"]}, bi, 40, 16)
    ec = compare_pieces({"Xinv": got["Xinv"]}, recs, bi)
    assert ec[("Xinv", "j0l0")] == pytest.approx(1e-9, rel=1e-3)
    assert all(v < 1e-30 for k, v in ec.items() if k != ("Xinv", "j0l0"))


@pytest.mark.parametrize("name", ["M-S", "M-T", "M-m"])
def test_restatement_fp64_mixed_per_piece(pk, cr, oracle, name):
    """One body of the restatement at words = 1 from the numpy oracle's state after 2 iterations:
    the new state per piece and mu, alpha_p, alpha_d, beta_c against the numpy oracle at the
    fp64 stage tolerance 1e-11 -- the tolerance of tests/test_gpu_mixed.py, held per piece by an
    independent implementation (Cholesky against the oracle's pivoted LU, other summation order).
    Measured worst piece, error / tolerance: M-S 5.2e-4 (x+ j3), M-T 7.7e-4 (Y+ j3l1),
    M-m 5.6e-4 (x+ j1)."""
    from helpers import stage_reference
    cons, b, bi, state, nxt, it = mixed_oracle_case(pk, oracle, name)
    ref = {k: v for k, v in stage_reference(it, nxt, bi).items() if k in STATE_KEYS + LOG_KEYS}
    got = _new_state(pk, cr, cons, b, pk.get_block_info(cons), 1, state)
    e = piecewise_err(got, ref, bi)
    assert len(e) == 2 * sum(bi.L) + bi.J + 1 + 4
    w, key = worst(e, 1e-11)
    print(f"{name}: worst error / tolerance {w:.3g} at {key}")
    bad = {k: v for k, v in e.items() if not v <= 1e-11}
    assert not bad, bad


@pytest.mark.parametrize("name,words,tol", [("mixdd", 2, 1e-25), ("mixdds", 2, 1e-25),
                                            ("mixqd", 4, 1e-50), ("mixqds", 4, 1e-50)])
def test_restatement_multiword_mixed_per_piece(pk, cr, fixtures, name, words, tol):
    """One body of the restatement at double-double / quad-double from the fixture state: the new
    state per piece and the logged mu, alpha_p, alpha_d, beta_c against the committed 256-bit
    per-piece records, at the tolerances tests/test_gpu_mixed.py asserts on the device (1e-25,
    1e-50), so that these are known to hold per piece for the reference algorithm at the
    device's precision.  Measured worst piece, error / tolerance: mixdd 2.0e-6 (x+ j1),
    mixdds 2.6e-6 (y+), mixqd 1.9e-14 (x+ j0), mixqds 2.2e-14 (x+ j0): the restatement needs no
    reference-error allowance (the max(tol, 16 ref_err) of the late-iterate test) on any piece."""
    sf = os.path.join(GOLDEN, f"stage_{name}.npz")
    cons, b = fixtures.instance(name, sf)
    bi = pk.get_block_info(cons)
    state = fixtures.load_state(sf, bi)
    with gzip.open(os.path.join(GOLDEN, f"stage_{name}_mp256.json.gz"), "rt") as f:
        fx = json.load(f)
    got = _new_state(pk, cr, cons, b, bi, words, state)
    recs = {k: fx["buffers"][k] for k in STATE_KEYS + LOG_KEYS}
    e = compare_pieces(got, recs, bi)
    w, key = worst(e, tol)
    print(f"{name} words={words}: worst error / tolerance {w:.3g} at {key}")
    bad = {k: v for k, v in e.items() if not v <= tol}
    assert not bad, bad


@pytest.mark.parametrize("name", ["mixdd", "mixdds", "mixqd", "mixqds"])
def test_mixed_fixture_consistency(pk, fixtures, name):
    """The committed records belong to the committed state and instance: every piece of
    helpers.stage_pieces has a record of its length; mu = <X, Y> / n of the stored fp64 state is
    the recorded mu to fp64 round-off; the instance regenerated by synth_mixed has the stored c
    and b; and no record file is larger than the largest uniform fixture."""
    from clrsdp_amd import instance as inst
    from helpers import mixed_instance
    sf = os.path.join(GOLDEN, f"stage_{name}.npz")
    cons, b = fixtures.instance(name, sf)
    cons0, b0 = mixed_instance(pk, name)
    assert np.array_equal(b, b0)
    assert all(np.array_equal(u.c, v.c) for u, v in zip(cons, cons0))
    bi = pk.get_block_info(cons)
    x, X, y, Y = fixtures.load_state(sf, bi)
    with gzip.open(os.path.join(GOLDEN, f"stage_{name}_mp256.json.gz"), "rt") as f:
        fx = json.load(f)
    assert fx["instance"] == name and fx["bits"] == 256 and fx["iters_before"] == 2
    size = lambda n: os.path.getsize(os.path.join(GOLDEN, f"stage_{n}_mp256.json.gz"))
    assert size(name) <= size("c4dd")
    for k, ps in stage_pieces(bi).items():
        assert set(fx["buffers"][k]) == {p[0] for p in ps}, k
        for piece, a, c in ps:
            assert fx["buffers"][k][piece]["n"] == c - a, (k, piece)
    mu = sum(float(np.sum(Xb * Yb)) for Xj, Yj in zip(X, Y) for Xb, Yb in zip(Xj, Yj)) / bi.total_dim
    with mpmath.workprec(256):
        ref = mpmath.mpf(fx["buffers"]["mu"]["all"]["val"][0])
        assert abs(mpmath.mpf(mu) - ref) <= 1e-13 * abs(ref)
