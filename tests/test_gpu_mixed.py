"""GPU stage parity on heterogeneous instances: clusters of different block sizes, dim_S, m, L
and sample ranks in one handle, compared per piece.

The device path builds its launch plans from handle-wide maxima and flags (build_plans and
build_fast_schur in csrc/clrsdp.hip) and gives every cluster and block its own branch and running
offset inside them.  pk.synth makes J identical clusters, so there the flags are all-or-nothing
and the offsets multiples of one stride; the instances here (helpers.MIXED, all
pk.synth_mixed(specs, n_y, seed=7)) mix them.  The metric is helpers.piecewise_err /
compare_pieces: every block, (r,s) slot and cluster relative to its own largest reference entry,
so an error confined to the small cluster cannot hide under the large cluster's scale.

fp64 against the numpy oracle at the state after 2 oracle iterations from initial_point(10, 10),
all ten stages at TOL64 = 1e-11: cond(S_j) is 13-88 and cond(Q) below 5 (M-Q: about 100) at the
compared states, the conditioning class of the 1e-11 tests of test_gpu_parity.py.  Multi-word
against the committed 256-bit per-piece fixtures (tests/golden/make_stage_fixtures.py) at 1e-25
(dd) and 1e-50 (qd); tests/test_cpu_mixed.py holds the CPU restatement to the same records.

Measured on an MI355X, worst piece of each instance as error / tolerance (every test prints it):
M-S 1.8e-3, M-S+ 2.5e-3, M-T 1.6e-3, M-Q 5.1e-3, M-m 1.4e-3, M-bS 2.9e-3, M-Bs 3.0e-3 (all at a
cluster's pred_dx; the switch and LU variants 1.3e-3 .. 2.4e-3), mixdd 8.1e-6, mixdds 1.8e-5,
mixqd and mixqds 5.1e-13.
"""
import gzip
import importlib.util
import json
import os

import numpy as np
import pytest

from helpers import (compare_pieces, mixed_instance, mixed_oracle_case, piecewise_err, residual_scales,
                     stage_device, stage_reference, worst)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL64 = 1e-11
PATH_SWITCHES = ("CLRSDP_SCHUR_FUSED", "CLRSDP_SCHUR_FUSED_ONE", "CLRSDP_SCHUR_FUSED_D64", "CLRSDP_SCHUR_FUSED_Y",
                 "CLRSDP_SCHUR_GRP2", "CLRSDP_CHOL256", "CLRSDP_CL_SOLVE", "CLRSDP_CHAIN")


def _mixed_compare(pk, oracle, monkeypatch, name, env=None, flags=None):
    """All ten stages of the handle of instance ``name`` against the numpy oracle, per piece at
    TOL64; every path switch unset (the library's own choice) except those of ``env``; ``flags``:
    clrsdp_set_factorization (the oracle factorises by pivoted LU, so the reference is the same)."""
    for k in PATH_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    cons, b, bi, state, nxt, it = mixed_oracle_case(pk, oracle, name)
    dev = pk.DeviceSolver(cons, b, pk.get_block_info(cons))
    try:
        if flags is not None:
            dev.set_factorization(flags)
            assert dev.factorization == flags
        dev.set_state(*state)
        got = stage_device(dev, False)
    finally:
        dev.close()
    e = piecewise_err(got, stage_reference(it, nxt, bi), bi, residual_scales(cons, b, state[1]))
    w, key = worst(e, TOL64)
    print(f"{name} {env or ''} {flags or ''}: {len(e)} pieces, worst error / tolerance {w:.3g} at {key}")
    bad = {k: v for k, v in e.items() if not v <= TOL64}
    assert not bad, f"per-piece stage parity failures: {bad}"


def test_mixed_single_and_2x2_schur_blocks(pk, oracle, monkeypatch):
    """M-S: m = 1, rank 1, blocks 20, 100, 70, 12, dim_S 39, 199, 139, 23, n_y = 24.
    reg_blk, reg_S, reg_Q and fac2 true.  The fac2 batch is mixed: a single-block cluster, a
    2 x 2-blocked one with D2 = 71, one with D2 = 11, and a single after them: s2off / b2off
    (advanced by the blocked clusters only), nc2 = 2 and the info slots of the second blocks,
    ci_S's order (both singles, then the S11 blocks).  fast_schur with every cluster direct,
    trivial_tuples and wa_fused true, n_gsum = 0; unequal block sizes, so uni_blk is false and the
    strip chains are off.  A delta <= 64 beside a delta > 64 rules out both fused forms, so the
    library's own choice is the unfused pair (test_mixed_schur_path_switches forces the others)."""
    _mixed_compare(pk, oracle, monkeypatch, "M-S")


def test_mixed_global_paths_with_small_riders(pk, oracle, monkeypatch):
    """M-S+: M-S and a fifth cluster with block 140 and dim_S 279.  reg_blk false (140 > 128) and
    reg_S false (279 > 256), so fac2 is false too: the blocks of 12..100 and the S_j of 23..199 ride
    the global-memory factorisations and solves sized for the large cluster; reg_Q true.  The
    fused Schur kernel is ruled out (delta = 140 > 128)."""
    _mixed_compare(pk, oracle, monkeypatch, "M-S+")


def test_mixed_tuple_shapes_in_one_fast_schur_handle(pk, oracle, monkeypatch):
    """M-T: m = 1, a rank-1 cluster (delta 40, direct), an all-rank-2 cluster (delta 33, grp2,
    ldG = dim_S), ranks 1, 2, 1, 3, 1, 2 (delta 24, gsum through the BX arena, ldG = K) and an
    L = 2 cluster with rank-0 samples (deltas 40 and 24, gsum); dim_S 79, 65, 47, 79, n_y = 24.
    reg_blk, reg_S, reg_Q, fac2 true, nc2 = 0.  fast_schur with t.G pointing at S (ld dim_S or
    K) or at the BX arena per descriptor; n_gsum = 2, so S is written in full (s_lower false
    although fac2 is true); trivial_tuples and wa_fused false because of the later clusters,
    although the first one is trivial.  any_grp2 with grp = 1 descriptors beside it: the fused
    kernel's group-sum epilogue is a template parameter of the whole launch (fused_grp2), so this
    handle must take the unfused pair, whose schur_pairs_f64 branches per descriptor.  (Every
    delta <= 64 and fewer than 128 row blocks, so by size alone the plan would take
    schur_fused_f64's ONE / D64 form; with fused_grp2 = any_grp2 that sums 2 x 2 groups of the
    rank-1 and unequal-rank clusters' tiles as well, and S of clusters 0, 2 and 3 is wrong.)"""
    _mixed_compare(pk, oracle, monkeypatch, "M-T")


def test_mixed_tuple_shapes_large_n_y(pk, oracle, monkeypatch):
    """M-Q: M-T at n_y = 140: reg_Q false (Q by the global-memory factorisation and solves) with
    reg_blk, reg_S and fac2 true and everything else on chip."""
    _mixed_compare(pk, oracle, monkeypatch, "M-Q")


def test_mixed_general_schur_large_blocks(pk, oracle, monkeypatch):
    """M-m: an m = 2, L = 2 cluster (blocks 60 and 40, dim_S 177) between two m = 1 clusters
    (blocks 70 and 100, dim_S 139 and 199), n_y = 24.  anyMgt1, so fast_schur is false and every
    cluster takes the general Schur assembly; d_blk_m (blocks 1 and 2) is a middle subset of
    d_blk; reg_blk, reg_S, reg_Q and fac2 true with nc2 = 3 (D2 = 11, 49, 71)."""
    _mixed_compare(pk, oracle, monkeypatch, "M-m")


def test_mixed_small_blocks_large_schur(pk, oracle, monkeypatch):
    """M-bS: an m = 3 cluster (block 90, dim_S 354) and an m = 1 cluster (block 20, dim_S 39),
    n_y = 16: reg_blk and reg_Q true, reg_S and fac2 false (354 > 256); anyMgt1."""
    _mixed_compare(pk, oracle, monkeypatch, "M-bS")


def test_mixed_large_block_small_schur(pk, oracle, monkeypatch):
    """M-Bs: block 140 with N = 150 samples (not 2 delta - 1; dim_S 150, 2 x 2-blocked with
    D2 = 22) and block 20 (dim_S 39), n_y = 16: reg_blk false, reg_S, reg_Q and fac2 true;
    fast_schur with the fused kernel ruled out (delta = 140 > 128)."""
    _mixed_compare(pk, oracle, monkeypatch, "M-Bs")


@pytest.mark.parametrize("switch,value", [("CLRSDP_SCHUR_FUSED", "0"), ("CLRSDP_SCHUR_FUSED", "1"),
                                          ("CLRSDP_SCHUR_FUSED_ONE", "0"), ("CLRSDP_SCHUR_FUSED_ONE", "1")])
@pytest.mark.parametrize("name", ["M-T", "M-S"])
def test_mixed_schur_path_switches(pk, oracle, monkeypatch, name, switch, value):
    """The Schur paths forced per handle on the mixed instances.  M-T (default: the unfused pair,
    schur_pairs_f64 summing the 2 x 2 groups of one cluster only): the same under all four
    settings -- FUSED=1 and FUSED_ONE=1 must not bring the fused kernel's handle-wide group-sum
    template back over the grp = 1 descriptors (test_mixed_rank2_cluster_through_gsum runs the
    fused kernel on this instance).  M-S (default: unfused, deltas 20 and 12 beside 100 and 70):
    FUSED=1 the multi-tile fused form with s_lower true (fac2, n_gsum = 0: only the lower
    triangle of S is assembled, FACTOR reads S21^T); FUSED_ONE=1 the padded ONE form on mixed
    deltas; FUSED=0 and FUSED_ONE=0 the unfused pair."""
    _mixed_compare(pk, oracle, monkeypatch, name, {switch: value})


def test_mixed_rank2_cluster_through_gsum(pk, oracle, monkeypatch):
    """M-T under CLRSDP_SCHUR_GRP2=0: the all-rank-2 cluster goes through the BX arena and
    schur_gsum like the unequal-rank ones: n_gsum = 3 and any_grp2 false, so the library takes
    schur_fused_f64 (ONE / D64 form, the plain template) with G at S (ld dim_S) for the direct
    cluster and in the BX arena (ld K) for the other four blocks in one launch."""
    _mixed_compare(pk, oracle, monkeypatch, "M-T", {"CLRSDP_SCHUR_GRP2": "0"})


@pytest.mark.parametrize("switch", ["CLRSDP_CHOL256", "CLRSDP_CL_SOLVE"])
def test_mixed_opt_in_factor_paths(pk, oracle, monkeypatch, switch):
    """M-S under CLRSDP_CHOL256=1 (S_j of 199 and 139 by one 768-thread workgroup beside the
    128-and-below instances of 39 and 23: nc2 = 0, the x4 slab and scratch sizing) and under
    CLRSDP_CL_SOLVE=1 (cl_solve_t / slab_qsolve / cl_solve_dx over clusters of 1 to 4 row blocks,
    two of them 2 x 2-blocked)."""
    _mixed_compare(pk, oracle, monkeypatch, "M-S", {switch: "1"})


@pytest.mark.parametrize("lu_x", [False, True], ids=["lu-sq", "lu-sq-x"])
@pytest.mark.parametrize("name", ["M-S", "M-m", "M-S+"])
def test_mixed_lu_factorisations(pk, oracle, monkeypatch, name, lu_x):
    """S_j and Q by pivoted LU (CLRSDP_FACT_LU_SQ), and X^-1 by LU as well (| CLRSDP_FACT_LU_X),
    on mixed sizes: the on-chip and the blocked LU in one batch (M-S+: blocks 12..140, S_j
    23..279).  The oracle factorises by pivoted LU, so reference and tolerance are unchanged."""
    from clrsdp_amd import _lib as L
    _mixed_compare(pk, oracle, monkeypatch, name, flags=L.FACT_LU_SQ | (L.FACT_LU_X if lu_x else 0))


@pytest.mark.parametrize("name", ["M-S", "M-S+", "M-T", "M-Q", "M-m", "M-bS", "M-Bs"])
def test_mixed_iterate_equals_stagewise(pk, monkeypatch, name):
    """clrsdp_iterate (the captured graph with its side-stream forks and joins) == the ten
    stages run one by one, bitwise, on every mixed plan: three bodies from the initial point."""
    from clrsdp_amd import _lib as L
    for k in PATH_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    cons, b = mixed_instance(pk, name)
    bi = pk.get_block_info(cons)
    P = pk.make_params("0.3", "0.1", "0.7", 0)
    st0 = pk.initial_point(bi, 10.0, 10.0)
    outs = []
    for mode in ("iterate", "stages"):
        dev = pk.DeviceSolver(cons, b, bi)
        try:
            dev.set_state(*st0)
            for _ in range(3):
                if mode == "iterate":
                    dev.iterate(P, False)
                else:
                    for s in range(L.NUM_STAGES):
                        dev.run_stage(s, P, False)
            outs.append(dev.get_state())
        finally:
            dev.close()
    a, c = outs
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[2], c[2])
    for j in range(bi.J):
        for l in range(bi.L[j]):
            assert np.array_equal(a[1][j][l], c[1][j][l]), (j, l)
            assert np.array_equal(a[3][j][l], c[3][j][l]), (j, l)


# ---- multi-word: the committed 256-bit per-piece fixtures ------------------------------------
def _fixture_module():
    spec = importlib.util.spec_from_file_location("make_stage_fixtures", os.path.join(GOLDEN, "make_stage_fixtures.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return M


def _mixed_fixture_compare(pk, name, words, tol):
    """Every stage of the handle of fixture ``name`` at ``words`` against its 256-bit per-piece
    records at ``tol`` (the CPU restatement holds it on the new state with five orders of margin
    or more, tests/test_cpu_mixed.py, so no buffer needs a reference-error allowance)."""
    M = _fixture_module()
    sf = os.path.join(GOLDEN, f"stage_{name}.npz")
    cons, b = M.instance(name, sf)
    bi = pk.get_block_info(cons)
    state = M.load_state(sf, bi)
    with gzip.open(os.path.join(GOLDEN, f"stage_{name}_mp256.json.gz"), "rt") as f:
        fx = json.load(f)
    dev = pk.DeviceSolver(cons, b, bi, precision_words=words)
    try:
        dev.set_state(*state)
        got = stage_device(dev, True)
    finally:
        dev.close()
    e = compare_pieces(got, fx["buffers"], bi, residual_scales(cons, b, state[1]))
    w, key = worst(e, tol)
    print(f"{name} words={words}: {len(e)} pieces, worst error / tolerance {w:.3g} at {key}")
    bad = {k: v for k, v in e.items() if not v <= tol}
    assert not bad, f"per-piece stage parity failures vs mp256: {bad}"


@pytest.mark.parametrize("variant", ["default", "full-pairs", "one-cu-potrf", "valu-products"])
def test_mixed_dd_global_paths(pk, variant, monkeypatch):
    """mixdd at double-double: blocks 12, 70, 40 and 24 (reg_blk false: 70 > 64), dim_S 23, 139,
    79 (reg_S and s_split false: 139 > 128), n_y = 70 (reg_Q and q_split false: Q by potrf and
    vector solves); the int8 (Ozaki) products with unequal delta and oz_kxoff per block, an L = 2
    cluster with rank-0 samples beside rank-1 ones.  The variants of
    test_stage_parity_dd_c4_shape: full pairings, the one-CU potrf, the VALU products."""
    for k, off in (("CLRSDP_MW_PAIR_UPPER", "full-pairs"), ("CLRSDP_POTRF_BLK", "one-cu-potrf"),
                   ("CLRSDP_OZAKI", "valu-products")):
        monkeypatch.delenv(k, raising=False)
        if variant == off:
            monkeypatch.setenv(k, "0")
    _mixed_fixture_compare(pk, "mixdd", 2, 1e-25)


def test_mixed_dd_split_form(pk, monkeypatch):
    """mixdds (mixdd without its large cluster) at double-double: dim_S 23 and 79, so reg_S is
    false and s_split true (79 <= 128) with a 23-wide S_j in the same split batch; reg_blk true
    (blocks 12, 40, 24); n_y = 70: reg_Q and q_split false."""
    for k in ("CLRSDP_MW_PAIR_UPPER", "CLRSDP_POTRF_BLK", "CLRSDP_OZAKI"):
        monkeypatch.delenv(k, raising=False)
    _mixed_fixture_compare(pk, "mixdds", 2, 1e-25)


def test_mixed_qd_m2_among_m1(pk):
    """mixqd at quad-double: an m = 2, L = 2 cluster (blocks 20 and 12, dim_S 57) after two m = 1
    clusters (blocks 8 and 36, dim_S 15 and 71): anyMgt1 (no upper-only pairings), reg_blk false
    (36 > 32), reg_S and s_split false (71 > 64), n_y = 40: reg_Q false, q_split true."""
    _mixed_fixture_compare(pk, "mixqd", 4, 1e-50)


def test_mixed_qd_split_form(pk):
    """mixqds (mixqd without its large cluster) at quad-double: dim_S 15 and 57, reg_S false and
    s_split true (57 <= 64) with a 15-wide S_j in the same batch; reg_blk true (blocks 8, 20, 12);
    q_split true (n_y = 40)."""
    _mixed_fixture_compare(pk, "mixqds", 4, 1e-50)
