"""The SCHUR-stage reference, bound and entry point without a GPU (tests/schur_cases.py):
  1. the generalised exact reference against the 256-bit oracle, against helpers.schur_dense and,
     bitwise, against the single-block helpers.schur_exact it generalises;
  2. the bound is attainable: a plain NumPy float64 restatement of the formula stays below it on
     every fp64 case of the tables of tests/test_gpu_schur.py (the largest ratio is printed and
     recorded in DESIGN.md §3), so the bound is not fitted to the device;
  3. the bound is sharp: every mistake of a list of plausible ones, applied to the reference
     itself, exceeds it on the random and exact classes at every width;
  4. clrsdp_schur_info is exported and refuses NULL arguments.
"""
import ctypes as C

import numpy as np
import pytest

import schur_cases as sc
from helpers import cw_err, graded_instance, schur_dense, schur_exact


def _mp_instance(pk, oracle, cons):
    ar = oracle.Mp(256)
    return ar, [pk.Cluster([[[ar.asarray(v) for v in vk] for vk in Al] for Al in cl.A], ar.asarray(cl.B),
                           ar.asarray(cl.c), [[[ar.num(x) for x in hk] for hk in Hl] for Hl in cl.H])
                for cl in cons]


def _ld_err(ld, ref, scale):
    """max |ld - ref| / scale of a longdouble array against mpf references, without rounding
    either to float64 (the reference goes in as a float64 pair)."""
    hi = np.array([float(v) for v in ref])
    lo = np.array([float(v - h) for v, h in zip(ref, hi)])
    ok = scale > 0
    return float(np.max((np.abs((ld - hi.astype(np.longdouble)) - lo) / np.where(ok, scale, 1))[ok]))


@pytest.mark.parametrize("specs", [
    [sc.sp(2, [5, 4], 6, sc.ranks_of("cyc", 2, 6)), sc.sp(1, [3], 4)],
    [sc.sp(1, [6, 4], 7, sc.ranks_of("cyc", 2, 7))],
], ids=["m2L2-mixed-ranks", "m1L2"])
def test_reference_matches_mp_oracle_and_dense(pk, oracle, specs):
    """schur_cases.schur_reference against oracle.Mp(256)'s S_raw and A_Y from the same 256-bit
    X^-1 (the oracle rounds every operation: 2^-240 of the bound scale), and against
    helpers.schur_dense from the float64 X^-1 (longdouble: 1e-17 of the scale)."""
    cons, b, bi, st, dec = sc.random_instance(pk, specs, 1)
    obi = oracle.get_block_info(cons)
    ar, consm = _mp_instance(pk, oracle, cons)
    Xi = oracle.xinv(ar, [[ar.asarray(M) for M in Xj] for Xj in st[1]])
    Ym = [[ar.asarray(M) for M in Yj] for Yj in st[3]]
    dec_o, AY_o = oracle.compute_T_decomposition(ar, consm, Xi, Ym, obi)
    S_o = np.concatenate([s.reshape(-1, order="F") for s in dec_o.S_raw])
    A_o = np.concatenate([AY_o[j][l][r][s] for j in range(bi.J) for l in range(bi.L[j])
                          for r in range(bi.m[j]) for s in range(r + 1)])
    S, AY, bS, bA = sc.schur_reference(cons, bi, Xi, st[3])
    assert len(S) == sum(D * D for D in bi.dim_S) and len(AY) == len(A_o)
    assert (bS > 0).any() and (bA > 0).all()
    assert sc.cw_ratio(S_o, S, bS) <= 2.0 ** -240
    assert sc.cw_ratio(A_o, AY, bA) <= 2.0 ** -240
    Xf = [[np.array(M, dtype=float) for M in Xj] for Xj in Xi]
    S2, AY2, bS2, bA2 = sc.schur_reference(cons, bi, Xf, st[3])
    S_d, AY_d = schur_dense(cons, bi, Xf, st[3])
    assert _ld_err(S_d, S2, bS2) <= 1e-17 and _ld_err(AY_d, AY2, bA2) <= 1e-17
    # the scales: the two routes to bS, bA agree to float64 round-off
    bS3, bA3 = sc.scales_only(cons, bi, Xf, st[3])
    assert np.allclose(bS3, bS2, rtol=1e-13, atol=0) and np.allclose(bA3, bA2, rtol=1e-13, atol=0)


@pytest.mark.parametrize("delta,rank,N,g", sc.GRADED)
def test_reference_is_bitwise_the_single_block_one(pk, delta, rank, N, g):
    """On the four cases of test_schur_products_componentwise_on_graded_data the generalised
    reference returns bitwise what helpers.schur_exact (unchanged) does: S, A_Y, bS, bA."""
    cons, b, st = graded_instance(pk, delta, rank, N, g, seed=21)
    Xi = np.linalg.inv(st[1][0][0])
    old = schur_exact(cons[0], Xi, st[3][0][0])
    new = sc.schur_reference(cons, pk.get_block_info(cons), [[Xi]], st[3], prec=256)
    for a, n in zip(old, new):
        assert len(a) == len(n)
        assert all(x == y for x, y in zip(a, n))


def test_exact53_is_exact_in_float64(pk):
    """The exact53 class: every intermediate fits 53 bits (span_bits), so the plain float64
    restatement equals the integer reference in every bit -- which is what lets the GPU tests
    take it as their reference at fp64 -- on a fused-size block, an L = 2 cluster and a cluster
    with ranks cycling through 0."""
    for specs in (sc._one(128, 65, 1), [sc.sp(1, (65, 40), 33)],
                  [sc.sp(1, [40], 33, sc.ranks_of("cyc", 1, 33))],
                  [sc.sp(2, [17], 17, sc.ranks_of(2, 1, 17))]):
        cons, b, bi, st, dec = sc.exact_instance(pk, specs, 1, small=True)
        Xi = [[np.diag(1.0 / np.diag(M)) for M in Xj] for Xj in st[1]]
        assert sc.span_bits(cons, bi, Xi, st[3]) <= 53
        S, AY, bS, bA = sc.schur_reference(cons, bi, Xi, st[3])
        S6, A6 = sc.schur_float64(cons, bi, Xi, st[3])
        assert all(float(x) == y for x, y in zip(S, S6)) and all(float(x) == y for x, y in zip(AY, A6))
        for Xj in st[1]:   # X = diag(4^i): its Cholesky factor and inverse are exact
            for M in Xj:
                Lc = np.linalg.cholesky(M)
                assert np.array_equal(Lc @ Lc.T, M) and np.array_equal(Lc, np.diag(np.sqrt(np.diag(M))))


def test_exact_classes_fit_their_words(pk):
    """exact53 fits the word on every case of the tables at every width (the GPU tests assert
    equality in every limb there); the exact class does at fp64 only for the smallest
    delta, which is why it is otherwise held to the componentwise bound."""
    worst = {}
    fits_exact = 0
    for c in sc.fp64_cases() + sc.general_cases() + sc.mw_cases():
        for small in (True, False):
            cons, b, bi, st, dec = sc.exact_instance(pk, c["specs"], c["words"], small=small)
            Xi = [[np.diag(1.0 / np.diag(M)) for M in Xj] for Xj in st[1]]
            bits = sc.span_bits(cons, bi, Xi, st[3])
            if small:
                assert sc.fits_word(bits, c["words"]), (c["id"], bits)
                worst[c["words"]] = max(worst.get(c["words"], 0), bits)
            else:
                fits_exact += sc.fits_word(bits, c["words"])
    print(f"exact53: widest intermediate {worst} bits; exact class fits its word on {fits_exact} cases")
    assert fits_exact > 0


def test_ozaki_plan_covers_exact53_and_not_exact(pk):
    """schur_cases.ozaki_covers on every int8 case of the multi-word table: the sixteen base-2^7
    digits cover the exact53 class (the GPU test then asserts equality in every limb on the int8
    products), and do not cover the exact class, whose 2^-70 term needs 12 digits per vector of V
    and more for V^T X^-1 V's second factor."""
    n = 0
    for c in sc.mw_cases():
        if not c["expect"].get("ozaki"):
            continue
        for small in (True, False):
            cons, b, bi, st, dec = sc.exact_instance(pk, c["specs"], 2, small=small)
            Xi = [[np.diag(1.0 / np.diag(M)) for M in Xj] for Xj in st[1]]
            assert sc.ozaki_covers(cons, bi, Xi, st[3]) == small, (c["id"], small)
        n += 1
    assert n == 36


_HOST_FP64 = sc.fp64_cases() + [c for c in sc.general_cases() if c["words"] == 1]


def test_bound_is_attainable_by_plain_float64(pk):
    """A plain NumPy float64 restatement of the formula (float64 GEMMs, Hadamard products,
    _sample_sums; X^-1 = numpy.linalg.inv(X), taken as the shared operand) meets the fp64 bound on
    every fp64 case of the GPU tables, random and exact classes.  The largest ratio is printed.
    The reference is the longdouble one on every case here (its error, 2^-9 of the bound, does not
    matter to ratios of 0.1; the integer form of the GPU tests would take minutes for all of
    them)."""
    worst = (0.0, None)
    for c in _HOST_FP64:
        for klass, inst in (("random", sc.random_instance(pk, c["specs"], 1)),
                            ("exact", sc.exact_instance(pk, c["specs"], 1))):
            cons, b, bi, st, dec = inst
            Xi = [[np.linalg.inv(M) for M in Xj] for Xj in st[1]]
            S, AY, bS, bA, how, bits = sc.reference_auto(cons, bi, Xi, st[3], 1, klass, ints=False)
            tS, tA = sc.tolerances(cons, bi, 1)
            S6, A6 = sc.schur_float64(cons, bi, Xi, st[3])
            hi = lambda a: np.array([float(v) for v in a]) if np.asarray(a).dtype == object else np.asarray(a)
            ok = bS > 0
            rS = float(np.max(np.abs(S6 - hi(S))[ok] / (bS * tS)[ok])) if ok.any() else 0.0
            rA = float(np.max(np.abs(A6 - hi(AY)) / (bA * tA)))
            assert np.all(S6[~ok] == 0)
            assert rS <= 1 and rA <= 1, (c["id"], klass, rS, rA)
            worst = max(worst, (rS, c["id"] + "/" + klass + "/S"), (rA, c["id"] + "/" + klass + "/A_Y"))
    print(f"float64 restatement: largest error / bound {worst[0]:.3g} at {worst[1]}")
    assert worst[0] > 1e-4  # (a bound a thousand times looser than what plain float64 needs is not one)


def _mutants(cons, bi, Xi, Y, Xi_dec, Y_dec, which):
    """{name: (S, A_Y)} of the reference with one mistake each."""
    ref = lambda **mut: sc.schur_reference(cons, bi, Xi, Y, mut=mut or None)[:2]
    S, AY = ref()
    N, D = bi.n_samples[0], bi.dim_S[0]
    out = {}
    delta = bi.Y_blocksizes[0][0] // bi.m[0]
    if "k" in which:
        out["last k-term dropped"] = ref(drop_k=delta - 1)
        out["k = 32 dropped"] = ref(drop_k=32)
        Sd = sc.schur_reference(cons, bi, Xi_dec, Y_dec)[0]
        for t in (64, 16):
            Sm = S.copy().reshape(-1)
            M, Md = Sm[:D * D].reshape(D, D), Sd[:D * D].reshape(D, D)
            M[:t, :t] = Md[:t, :t]
            out[f"{t} x {t} tile left at the decoy's value"] = (Sm, AY)
        lam = [float(x) for hk in cons[0].H[0] for x in hk]
        out["one lambda factor omitted"] = ref(lam=int(np.argmax(np.array(lam) != 1.0)))
        out["A_Y shifted by one column"] = (S, np.roll(AY, 1))
        Sm = S.copy().reshape(-1)
        M = Sm[:D * D].reshape(D, D)
        h = N // 2
        ev, od = slice(0, 2 * h, 2), slice(1, 2 * h, 2)
        M[:h, :h] = M[ev, ev] + M[od, ev] + M[ev, od] + M[od, od]
        out["group sum applied to a rank-1 cluster"] = (Sm, AY)
    if "m" in which:
        out["1/4 omitted"] = ref(quarter=1)
        out["BY untransposed"] = ref(by_untransposed=1)
    if "g" in which:
        out["one term of a 2 x 2 rank group omitted"] = ref(group_term=1)
    return (S, AY), out


@pytest.mark.parametrize("words", [1, 2, 4])
@pytest.mark.parametrize("klass", ["random", "exact"])
def test_bound_is_sharp(pk, words, klass):
    """Applied to the reference result, each of these exceeds the bound: a dropped last k-term, a
    dropped term k = 32, one 64 x 64 and one 16 x 16 tile left at the decoy's value, one lambda
    factor omitted, A_Y shifted by one column, the group sum applied to a rank-1 cluster (m = 1,
    delta = 40, K = 70); the 1/4 omitted and BY taken untransposed (m = 2); one term of a 2 x 2
    rank group omitted (rank 2).  X^-1 is inv(X) in float64 (diagonal, exact, on the exact
    class)."""
    for which, specs in (("k", sc._one(40, 70, 1)), ("m", [sc.sp(2, [5], 6)]), ("g", sc._one(8, 10, 2))):
        make = sc.random_instance if klass == "random" else sc.exact_instance
        inst = make(pk, specs, words)
        cons, b, bi, st, dec = inst
        inv = lambda X: [[np.linalg.inv(np.array(M, dtype=float)) for M in Xj] for Xj in X]
        (S, AY), muts = _mutants(cons, bi, inv(st[1]), st[3], inv(dec[1]), dec[3], which)
        bS, bA = sc.schur_reference(cons, bi, inv(st[1]), st[3])[2:]
        tS, tA = sc.tolerances(cons, bi, words)
        assert sc.cw_ratio(S, S, bS * tS) == 0
        for name, (Sm, Am) in muts.items():
            r = max(sc.cw_ratio(Sm, S, bS * tS), sc.cw_ratio(Am, AY, bA * tA))
            assert r > 1, (name, klass, words, r)


def test_schur_info_is_exported_and_refuses_null(pk):
    from clrsdp_amd import _lib as L
    assert "clrsdp_schur_info" in L.EXPORTS
    lib = L.lib()
    assert lib.clrsdp_schur_info.restype is C.c_int32
    assert C.sizeof(L.SchurInfo) == 13 * 4
    assert callable(pk.DeviceSolver.schur_info)
    out = L.SchurInfo()
    assert lib.clrsdp_schur_info(None, C.byref(out)) == L.E_ARG
    # (a NULL `out` is refused before the handle is looked at: the handle here is never read)
    dummy = C.create_string_buffer(64)
    assert lib.clrsdp_schur_info(C.cast(dummy, C.c_void_p), None) == L.E_ARG
