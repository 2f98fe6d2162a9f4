"""GPU tests of every product kernel on its own (clrsdp_gemm / solver.gemm, include/clrsdp.h):
gemm_f64_uni (64 and 32 tiles), gemm_f64_lds, gemm_f64_dyn, gemm_valu_ks at double-double and
quad-double, and the five code paths of gemv_batched, at the smallest shapes that straddle each
kernel's internal boundaries (tile 64 / 32 / 8, K-slab 32, MFMA k-step 4, the 128 / 32 / 16 / 4
ladders of the GEMV), with every leading dimension also at rows + 3.

Every test asserts the kernel the plan launched (``path``), compares each result with the exact
product of tests/gemm_cases.py in mpmath at 320 bits against the componentwise a-priori bound
(K + 4) u (|alpha| |op A||op B| + |beta C_in| + |dmult s| I) (K + 6 for the scaled-A form), and
checks that the result holds no NaN although every padding row of A, B and C_in does, and that the
padding rows, gaps and guard zones of C come back bitwise.  The operand classes random, graded and
cancelling share each batch; one exact case per path must be the reference in every limb, also
with A scaled by 2^+-400.  Every test prints the largest ratio to the bound.

The sensitivity of these checks is shown without a GPU by tests/test_gemm_host.py."""
import numpy as np
import pytest

import gemm_cases as gc

pytestmark = pytest.mark.gpu

KINDS3 = ("random", "graded", "cancel")
# (M, N, K): tile 64 or 32, K-slab 32, MFMA k-step 4
SHAPES = [(1, 1, 1), (1, 65, 3), (65, 1, 5), (31, 33, 4), (32, 32, 32), (33, 31, 33), (63, 65, 31),
          (64, 64, 64), (65, 63, 65), (129, 70, 97), (70, 129, 36), (128, 128, 128)]
TRANS = [(False, False), (True, False), (False, True), (True, True)]
TRANS_IDS = ["NN", "TN", "NT", "TT"]
# (alpha, beta, where C_in lives)
CMODES = [(1.0, 0.0, None), (1.0, -1.0, "inplace"), (2.0, 0.5, "separate")]
CMODE_IDS = ["beta0", "beta-1-inplace", "beta0.5-separate"]
_cache = {}


def _ops(kind, M, N, K, words, seed=21):
    """(op(A), op(B), exact product) of one problem, computed once and left unchanged"""
    key = (kind, M, N, K, words, seed)
    if key not in _cache:
        A, B = gc.operands(kind, M, N, K, words, seed)
        A.setflags(write=False)
        B.setflags(write=False)
        _cache[key] = (A, B, gc.product(A, B))
    return _cache[key]


def _cin(kind, M, N, words, seed=21):
    key = ("cin", kind, M, N, words, seed)
    if key not in _cache:
        _cache[key] = gc.matrix(kind, M, N, words, seed)
        _cache[key].setflags(write=False)
    return _cache[key]


def _run(pk, specs, words, expect, label, form="plain", ta=False, tb=False, alpha=1.0, beta=0.0,
         cmode=None, ldpad=0, gaps=None, dscal=None, dmult=0.0, check=None, seed=21):
    """one launch of the problems ``specs`` = [(kind, M, N, K)], every result against its bound;
    ``check(p, got, ref, bnd)`` replaces the full comparison (it returns the ratio)"""
    from clrsdp_amd import _lib as L
    data = [_ops(k, M, N, K, words, seed) for k, M, N, K in specs]
    cins = [_cin(k, M, N, words, seed) for k, M, N, K in specs] if cmode else None
    res = pk.gemm([gc.stored(d[0], ta) for d in data], [gc.stored(d[1], tb) for d in data], Cin=cins,
                  precision_words=words, form=form, transa=ta, transb=tb, alpha=alpha, beta=beta,
                  dscal=dscal, dmult=dmult, inplace=cmode == "inplace", ldpad=ldpad, gaps=gaps,
                  raw_limbs=True)
    assert res.path == expect, f"{label}: ran {L.PATH_NAMES.get(res.path, res.path)}, " \
                               f"written for {L.PATH_NAMES[expect]}"
    assert res.untouched, f"{label}: the padding, a gap or a guard zone of C was written"
    diag = dmult * dscal if dscal is not None else 0.0
    worst = 0.0
    for p, ((kind, M, N, K), (A, B, P)) in enumerate(zip(specs, data)):
        ci = cins[p] if cmode else None
        ref = gc.reference_ints(P, alpha, beta, ci, diag)
        bnd = gc.bound(A, B, words, alpha, beta, ci, diag)
        r = check(p, res.C[p], ref, bnd) if check else gc.ratio(res.C[p], ref, bnd)
        assert r <= 1.0, f"{label}: problem {p} {specs[p]}: error / bound = {r:.3e}"
        worst = max(worst, r)
    print(f"GEMM {L.PATH_NAMES[expect]} words={words} {label}: error / bound = {worst:.3e}")
    return res


def _three(shape):
    return [(k,) + tuple(shape) for k in KINDS3]


# ---- fp64 tiled kernels -------------------------------------------------------------------------
@pytest.mark.parametrize("cm", CMODES, ids=CMODE_IDS)
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
def test_lds_whole_set(pk, ta, tb, cm):
    """gemm_f64_lds: the whole shape set in the three operand classes as one non-uniform batch"""
    from clrsdp_amd import _lib as L
    alpha, beta, cmode = cm
    specs = [(k,) + s for k in KINDS3 for s in SHAPES]
    for ldpad in (0, 3):
        _run(pk, specs, 1, L.PATH_LDS, f"lds {ta=} {tb=} {cm=} {ldpad=}", ta=ta, tb=tb, alpha=alpha,
             beta=beta, cmode=cmode, ldpad=ldpad)


def _uni_path(L, M, N, K, ta, tb, tile):
    if N == 1 and (not tb or K == 1):            # a batch of matrix-vector products
        return L.PATH_GEMV_T_F64 if ta else L.PATH_GEMV_N_F64
    return L.PATH_UNI64 if tile == 64 else L.PATH_UNI32


@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
@pytest.mark.parametrize("tile", [64, 32])
def test_uni_each_shape(pk, monkeypatch, tile, ta, tb):
    """gemm_f64_uni: every shape as a uniform batch of three (one per operand class), 64-tiles
    (CLRSDP_GEMM_TS32_BELOW=0) and 32-tiles (a large threshold); the diagonal scalar with dmult and
    a separate C_in on the square shapes.  The two N = 1 shapes are matrix-vector batches and take
    gemv_batched (with transb only at K = 1); the diagonal scalar is not defined there."""
    from clrsdp_amd import _lib as L
    monkeypatch.setenv("CLRSDP_GEMM_TS32_BELOW", "0" if tile == 64 else "1000000")
    for s in SHAPES:
        path = _uni_path(L, *s, ta, tb, tile)
        for ldpad in (0, 3):
            _run(pk, _three(s), 1, path, f"uni{tile} {s} {ta=} {tb=} {ldpad=}", ta=ta, tb=tb, ldpad=ldpad)
        _run(pk, _three(s), 1, path, f"uni{tile} {s} {ta=} {tb=} in place", ta=ta, tb=tb, alpha=1.0,
             beta=-1.0, cmode="inplace", ldpad=3)
        if s[0] == s[1] and s[1] > 1:
            _run(pk, _three(s), 1, path, f"uni{tile} {s} {ta=} {tb=} +sI", ta=ta, tb=tb, alpha=2.0,
                 beta=0.5, cmode="separate", dscal=0.75, dmult=-1.0)


@pytest.mark.parametrize("arena", ["A", "B", "C", "Cin"])
def test_uniform_detection(pk, monkeypatch, arena):
    """the same three problems at equal strides (gemm_f64_uni) and with the second problem moved
    by one element in one arena (gemm_f64_lds): both meet the bound"""
    from clrsdp_amd import _lib as L
    monkeypatch.setenv("CLRSDP_GEMM_TS32_BELOW", "0")
    specs = _three((65, 63, 65))
    kw = dict(alpha=2.0, beta=0.5, cmode="separate", ldpad=3)
    _run(pk, specs, 1, L.PATH_UNI64, "equal strides", **kw)
    _run(pk, specs, 1, L.PATH_UNI64, f"equal gaps in {arena}", gaps={arena: [2, 2, 2]}, **kw)
    _run(pk, specs, 1, L.PATH_LDS, f"{arena} moved by one", gaps={arena: [0, 1, 0]}, **kw)
    monkeypatch.delenv("CLRSDP_GEMM_TS32_BELOW")
    _run(pk, specs, 1, L.PATH_UNI32, "default threshold: 6 tiles of 64 < 192", **kw)


SYM_N = [1, 31, 32, 33, 64, 65, 97, 129]


def _sym_data(n, tb, same, seed):
    """A = L^-1-like lower triangular; B symmetric (as q_sx2 has it), or with `same` B = A and
    transb, so that the exact product A A^T is symmetric"""
    key = ("sym", n, tb, same, seed)
    if key not in _cache:
        A = gc.known_lower(n, seed)[None]
        B = A if same else gc.sym_matrix(n, seed)[None]
        opB = np.ascontiguousarray(B.transpose(0, 2, 1)) if tb else B
        _cache[key] = (A, B, gc.product(A, opB), opB)
    return _cache[key]


def _sym_check(pk, ns_batches, tb, expect, label):
    from clrsdp_amd import _lib as L
    for same in ((False, True) if tb else (False,)):
        for ns in ns_batches:
            data = [_sym_data(n, tb, same, 30 + q) for q, n in enumerate(ns)]
            res = pk.gemm([d[0] for d in data], [d[1] for d in data], form="sym", transb=tb,
                          raw_limbs=True)
            path = expect(ns)
            assert res.path == path, (label, ns, L.PATH_NAMES.get(res.path))
            assert res.untouched
            worst = 0.0
            for (A, B, P, opB), got in zip(data, res.C):
                assert not np.isnan(got).any()
                assert np.array_equal(got[0], got[0].T), f"{label}: n={A.shape[1]} not bitwise symmetric"
                ref, bnd = gc.reference_ints(P), gc.bound(A, opB, 1)
                # L M is not symmetric: the computed half is the lower triangle
                r = gc.ratio(got, ref, bnd, mask=None if same else np.tri(A.shape[1], dtype=bool))
                assert r <= 1.0, (label, ns, same, r)
                worst = max(worst, r)
            print(f"GEMM SYM {L.PATH_NAMES[path]} {label} {same=} n={ns}: error / bound = {worst:.3e}")


@pytest.mark.parametrize("tb", [False, True], ids=["NN", "NT"])
@pytest.mark.parametrize("variant", ["uni64", "uni32", "lds"])
def test_sym(pk, monkeypatch, variant, tb):
    """the SYM epilogue: the result meets the bound on the half the kernel computes (everywhere
    when the exact product is symmetric) and is bitwise symmetric.  A uniform batch of 1 x 1
    problems is a matrix-vector batch (gemv_batched; trivially symmetric)."""
    from clrsdp_amd import _lib as L
    if variant == "lds":
        _sym_check(pk, [SYM_N], tb, lambda ns: L.PATH_LDS, "lds")
        return
    monkeypatch.setenv("CLRSDP_GEMM_TS32_BELOW", "0" if variant == "uni64" else "1000000")
    tiled = L.PATH_UNI64 if variant == "uni64" else L.PATH_UNI32
    _sym_check(pk, [[n] * 3 for n in SYM_N], tb,
               lambda ns: L.PATH_GEMV_N_F64 if ns[0] == 1 else tiled, variant)


SCA_MN, SCA_K = [1, 33, 64, 100], [1, 31, 33, 65, 199]


def _scaled(pk, specs, expect, label, seed=41):
    from clrsdp_amd import _lib as L
    data = [_ops(k, M, N, K, 1, seed) for k, M, N, K in specs]
    sa = [gc._uniform(seed, 80 + p, (s[3],)) for p, s in enumerate(specs)]
    sl = [1.0 + 0.5 * gc._uniform(seed, 300 + p, (s[3],)) for p, s in enumerate(specs)]
    res = pk.gemm([d[0] for d in data], [gc.stored(d[1], True) for d in data], form="scaled",
                  transb=True, sa=sa, sl=sl, ldpad=3, raw_limbs=True)
    assert res.path == expect, (label, L.PATH_NAMES.get(res.path))
    assert res.untouched
    worst = 0.0
    for p, (A, B, _) in enumerate(data):
        ref = gc.reference_ints(gc.product(A, B, scale=(sa[p], sl[p])))
        r = gc.ratio(res.C[p], ref, gc.bound(A, B, 1, extra=6, scale=(sa[p], sl[p])))
        assert r <= 1.0, (label, specs[p], r)
        worst = max(worst, r)
    print(f"GEMM SCALED {L.PATH_NAMES[expect]} {label}: error / bound = {worst:.3e}")


@pytest.mark.parametrize("variant", ["uni64", "uni32", "lds"])
def test_scaled(pk, monkeypatch, variant):
    """the scaled-A form A diag(sa sl) B^T (the weighted-A products): never a GEMV, also at 1 x 1"""
    from clrsdp_amd import _lib as L
    if variant == "lds":
        specs = [(KINDS3[(i + j) % 3], n, n, K) for i, n in enumerate(SCA_MN) for j, K in enumerate(SCA_K)]
        _scaled(pk, specs, L.PATH_LDS, "all shapes")
        return
    monkeypatch.setenv("CLRSDP_GEMM_TS32_BELOW", "0" if variant == "uni64" else "1000000")
    for n in SCA_MN:
        for K in SCA_K:
            _scaled(pk, _three((n, n, K)), L.PATH_UNI64 if variant == "uni64" else L.PATH_UNI32,
                    f"{variant} n={n} K={K}")


def test_mixed(pk):
    """gemm_f64_dyn: one batch with the four transposes and per problem (alpha, beta) = (1, 0),
    (-1, 1) in place, (-1, 0) with the diagonal flag, (2, 0.5) with a separate C_in, on unequal
    shapes (XINV's and FACTOR's usage)"""
    from clrsdp_amd import _lib as L
    squares = [s for s in SHAPES if s[0] == s[1]]
    combos = [(1.0, 0.0, 0, None), (-1.0, 1.0, 0, "inplace"), (-1.0, 0.0, 1, None), (2.0, 0.5, 0, "separate")]
    specs, ops, cins, inpl = [], [], [], []
    for t, (ta, tb) in enumerate(TRANS):
        for c, (al, be, dg, cmode) in enumerate(combos):
            q = 4 * t + c
            s = squares[(t + c) % 4] if dg else SHAPES[(3 * q + 1) % len(SHAPES)]
            specs.append((KINDS3[q % 3],) + s)
            ops.append((ta, tb, al, be, dg))
            cins.append(_cin(specs[-1][0], s[0], s[1], 1) if cmode else None)
            inpl.append(cmode == "inplace")
    data = [_ops(*sp, 1) for sp in specs]
    sval = 0.625
    for ldpad in (0, 3):
        res = pk.gemm([gc.stored(d[0], o[0]) for d, o in zip(data, ops)],
                      [gc.stored(d[1], o[1]) for d, o in zip(data, ops)], Cin=cins, form="mixed",
                      ops=ops, inplace=inpl, dscal=sval, ldpad=ldpad, raw_limbs=True)
        assert res.path == L.PATH_DYN, L.PATH_NAMES.get(res.path)
        assert res.untouched
        worst = 0.0
        for p, ((A, B, P), (ta, tb, al, be, dg)) in enumerate(zip(data, ops)):
            diag = sval if dg else 0.0
            ref = gc.reference_ints(P, al, be, cins[p], diag)
            r = gc.ratio(res.C[p], ref, gc.bound(A, B, 1, al, be, cins[p], diag))
            assert r <= 1.0, (specs[p], ops[p], r)
            worst = max(worst, r)
        print(f"GEMM {L.PATH_NAMES[L.PATH_DYN]} mixed batch {ldpad=}: error / bound = {worst:.3e}")


@pytest.mark.parametrize("words", [1, 2, 4], ids=["fp64", "dd", "qd"])
def test_one_column_with_transb(pk, words):
    """N = 1 with op(B) = B^T: the 1 x K row is the GEMV's vector only at K = 1 (the comment in
    GemmPlan::finalize); K > 1 must take a tiled kernel"""
    from clrsdp_amd import _lib as L
    tiled = L.PATH_LDS if words == 1 else L.PATH_VALU_KS
    gemv = L.PATH_GEMV_N_F64 if words == 1 else L.PATH_GEMV_N_MW
    _run(pk, [("random", 65, 1, 5), ("graded", 33, 1, 4)], words, tiled, "N=1 NT K>1", tb=True, ldpad=3)
    _run(pk, [("random", 65, 1, 1), ("graded", 33, 1, 1)], words, gemv, "N=1 NT K=1", tb=True, ldpad=3)
    _run(pk, [("random", 65, 1, 5), ("graded", 33, 1, 1)], words, tiled, "N=1 NT K mixed", tb=True)
    _run(pk, [("random", 65, 1, 5), ("graded", 33, 1, 4)], words, gemv, "N=1 NN K>1", tb=False, ldpad=3)


def test_a_refused_device_leaves_no_error_behind(pk):
    """a call on a device that does not exist is CLRSDP_E_HIP, and the HIP runtime's per-thread
    last error is cleared with it: the launch check of the next, good call used to report it (the
    first GPU test after tests/test_gemm_host.py failed with "invalid device ordinal")"""
    from clrsdp_amd import _lib as L
    A, B, _ = _ops("random", 9, 8, 5, 1)
    for bad in (lambda: pk.gemm([A], [B], device=1 << 20),
                lambda: pk.gemm_chain("chain", [np.eye(4)], [np.eye(4)], [np.eye(4)], device=1 << 20),
                lambda: pk.potrf([np.eye(4)], device=1 << 20)):
        with pytest.raises(L.ClrsdpError) as ei:
            bad()
        assert ei.value.code == L.E_HIP
        _run(pk, [("random", 9, 8, 5)], 1, L.PATH_UNI32, "after a refused device")
        O, _ = pk.gemm_chain("chain", [np.eye(4)], [2.0 * np.eye(4)], [np.eye(4)])
        assert np.array_equal(O[0], 2.0 * np.eye(4))


# ---- gemm_valu_ks -------------------------------------------------------------------------------
KS_MN = {2: [1, 7, 8, 9, 17], 4: [1, 8, 9, 17]}
KS_K = {2: [1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 65], 4: [1, 4, 5, 9, 31, 33, 65]}


@pytest.mark.parametrize("cm", CMODES, ids=CMODE_IDS)
@pytest.mark.parametrize("ta,tb", TRANS, ids=TRANS_IDS)
@pytest.mark.parametrize("words", [2, 4], ids=["dd", "qd"])
def test_valu_ks(pk, words, ta, tb, cm):
    """gemm_valu_ks: 8 x 8 tiles, 32-k chunks, k split mod 4 in two chains (the quad-double grid
    is thinned)"""
    from clrsdp_amd import _lib as L
    alpha, beta, cmode = cm
    specs = [(KINDS3[(i + j + l) % 3], M, N, K) for i, M in enumerate(KS_MN[words])
             for j, N in enumerate(KS_MN[words]) for l, K in enumerate(KS_K[words])]
    for ldpad in (0, 3):
        _run(pk, specs, words, L.PATH_VALU_KS, f"valu_ks {ta=} {tb=} {cm=} {ldpad=}", ta=ta, tb=tb,
             alpha=alpha, beta=beta, cmode=cmode, ldpad=ldpad)


@pytest.mark.parametrize("words", [2, 4], ids=["dd", "qd"])
def test_upper(pk, words):
    """the `upper` tile list: every 8 x 8 tile on or above the diagonal meets the bound (so every
    element with i <= j does), every tile strictly below it still holds the payload NaN"""
    from clrsdp_amd import _lib as L
    from clrsdp_amd.solver import GEMM_PAYLOAD
    specs = [(KINDS3[(i + l) % 3], n, n, K) for i, n in enumerate([1, 8, 9, 23]) for l, K in enumerate([1, 5, 33])]

    def check(p, got, ref, bnd):
        n = got.shape[1]
        tm, tn = np.arange(n)[:, None] // 8, np.arange(n)[None, :] // 8
        below = np.broadcast_to(tm > tn, (n, n))
        assert np.all(got.view(np.uint64)[:, below] == GEMM_PAYLOAD), f"problem {p}: a tile below the diagonal was written"
        assert not np.isnan(got[:, ~below]).any()
        assert np.all(~below[np.triu_indices(n)])
        return gc.ratio(got, ref, bnd, mask=~below)

    for tb in (False, True):
        for ldpad in (0, 3):
            _run(pk, specs, words, L.PATH_VALU_KS, f"upper {tb=} {ldpad=}", form="upper", tb=tb,
                 ldpad=ldpad, check=check)


# ---- gemv_batched -------------------------------------------------------------------------------
GEMV_M = [1, 63, 64, 65, 130]
GEMV_K = [1, 2, 4, 5, 15, 16, 17, 31, 32, 33, 112, 113, 127, 128, 129, 131, 260]


@pytest.mark.parametrize("ta", [False, True], ids=["N", "T"])
@pytest.mark.parametrize("words", [1, 2, 4], ids=["fp64", "dd", "qd"])
def test_gemv(pk, words, ta):
    """every path of gemv_batched: K at the ends of the 128, 32, 16 and 4 ladders, M around the
    64 outputs of a workgroup, one batch per (words, transa), beta = 0 and -1 in place, lda = rows + 3"""
    from clrsdp_amd import _lib as L
    path = {(1, False): L.PATH_GEMV_N_F64, (1, True): L.PATH_GEMV_T_F64, (2, False): L.PATH_GEMV_N_MW,
            (4, False): L.PATH_GEMV_N_MW, (2, True): L.PATH_GEMV_T_DD, (4, True): L.PATH_GEMV_T_QD}[(words, ta)]
    specs = [(KINDS3[(i + l) % 3], M, 1, K) for i, M in enumerate(GEMV_M) for l, K in enumerate(GEMV_K)]
    _run(pk, specs, words, path, f"gemv {ta=} beta=0", ta=ta, ldpad=3)
    _run(pk, specs, words, path, f"gemv {ta=} beta=-1 in place", ta=ta, beta=-1.0, cmode="inplace", ldpad=3)


# ---- one exact case per path --------------------------------------------------------------------
EXACT = [
    ("gemv_n_f64", 1, dict(), [(65, 1, 131)] * 2, "PATH_GEMV_N_F64"),
    ("gemv_t_f64", 1, dict(ta=True), [(65, 1, 131)] * 2, "PATH_GEMV_T_F64"),
    ("gemv_n_dd", 2, dict(), [(65, 1, 37)] * 2, "PATH_GEMV_N_MW"),
    ("gemv_n_qd", 4, dict(), [(65, 1, 37)] * 2, "PATH_GEMV_N_MW"),
    ("gemv_t_dd", 2, dict(ta=True), [(65, 1, 37)] * 2, "PATH_GEMV_T_DD"),
    ("gemv_t_qd", 4, dict(ta=True), [(65, 1, 37)] * 2, "PATH_GEMV_T_QD"),
    ("uni64", 1, dict(tb=True, env="0"), [(65, 63, 65)] * 2, "PATH_UNI64"),
    ("uni32", 1, dict(tb=True, env="1000000"), [(65, 63, 65)] * 2, "PATH_UNI32"),
    ("lds", 1, dict(ta=True), [(65, 63, 65), (33, 31, 33)], "PATH_LDS"),
    ("dyn", 1, dict(form="mixed"), [(65, 63, 65), (33, 31, 33)], "PATH_DYN"),
    ("valu_ks_dd", 2, dict(tb=True), [(17, 9, 65), (9, 17, 33)], "PATH_VALU_KS"),
    ("valu_ks_qd", 4, dict(ta=True), [(17, 9, 65), (9, 17, 33)], "PATH_VALU_KS"),
]


@pytest.mark.parametrize("case", EXACT, ids=[c[0] for c in EXACT])
def test_exact_case_per_path(pk, monkeypatch, case):
    """small integers times powers of two: every partial sum is representable whatever the order,
    so C = 2 op(A) op(B) + 0.5 C_in must equal the reference in every limb (compared as numbers:
    a zero limb may carry either sign), and again with A and C_in scaled by 2^400 and 2^-400"""
    from clrsdp_amd import _lib as L
    name, words, kw, shapes, pname = case
    kw = dict(kw)
    if "env" in kw:
        monkeypatch.setenv("CLRSDP_GEMM_TS32_BELOW", kw.pop("env"))
    ta, tb, form = kw.get("ta", False), kw.get("tb", False), kw.get("form", "plain")
    for sc in (1.0, 2.0 ** 400, 2.0 ** -400):
        data = [_ops("exact", M, N, K, words, 50 + p) for p, (M, N, K) in enumerate(shapes)]
        cins = [_cin("exact", M, N, words, 50 + p) * sc for p, (M, N, K) in enumerate(shapes)]
        ops = [(ta, tb, 2.0, 0.5, 0)] * len(shapes) if form == "mixed" else None
        res = pk.gemm([gc.stored(d[0] * sc, ta) for d in data], [gc.stored(d[1], tb) for d in data],
                      Cin=cins, precision_words=words, form=form, transa=ta, transb=tb, alpha=2.0,
                      beta=0.5, ops=ops, ldpad=3, raw_limbs=True)
        assert res.path == getattr(L, pname), L.PATH_NAMES.get(res.path)
        assert res.untouched
        for p, (A, B, P) in enumerate(data):
            ref = gc.reference(gc.product(A * sc, B), 2.0, 0.5, cins[p])
            want = gc.split(ref, words)
            assert np.array_equal(res.C[p], want), \
                f"{name} scale {sc:g} problem {p}: {int(np.sum(res.C[p] != want))} limbs differ"
