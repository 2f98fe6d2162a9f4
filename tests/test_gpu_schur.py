"""GPU tests of the SCHUR stage on every row of its dispatch table (schur_fused_f64 in its eight
instantiations, schur_pairs_f64, schur_gsum, schur_assemble in both forms, extract_AY, oz_split /
oz_gemm), through the handle: STAGE_MU_R, STAGE_XINV, STAGE_SCHUR, then S and A_Y against the
exact reference of tests/schur_cases.py under its componentwise bound
    |S - S_ref| <= (8 (delta_max + 2) + 2 T) u bS,   |A_Y - A_Y_ref| <= 8 (delta_max + 2) u bA
(derivation, operand classes and the case tables: the docstring of tests/schur_cases.py).

Stale-data rule.  Every handle runs the stage first on a decoy state (the same instance with X, Y
of another seed, scaled by 8) and then on the case's state; only the second result is compared.
An entry the kernels do not write then carries a wrong finite value, not an accident of the
allocator.

Path rule.  Every case asserts DeviceSolver.schur_info() against the row it claims to test.

Both triangles.  The rows marked with a dagger in DESIGN.md §3 run twice: with the default flags,
where the fused kernel stores the lower triangle only (s_lower = 1 when every dim_S <= 256 and no
cluster is summed by schur_gsum) and the upper triangle of BUF_S as read here is the host's
mirror; and with FACT_LU_SQ, where full = 1 and s_lower = 0 are asserted, both triangles of the
raw BUF_S are compared with the reference, and they must be bitwise each other's mirror wherever
the kernel writes S directly from one value (L = 1 with every rank 1, or every rank 2 with the
group sums in the kernel).

Every test prints its largest error / bound per class ("SCHUR ..." lines); DESIGN.md §3 carries
the table.  The natural multi-tile choice (at least 128 row blocks in the batch) stays with
test_c3_full_size_newton_identities.
"""
import numpy as np
import pytest

import schur_cases as sc

pytestmark = pytest.mark.gpu

_REF = {}


def _direct(c, j):
    """Cluster j's S_j is written by the pairing kernel itself from one value per entry pair."""
    s = c["specs"][j]
    if len(s["deltas"]) != 1 or s["m"] != 1:
        return False
    r = s["ranks"]
    if r is None or all(x == 1 for x in r[0]):
        return True
    return all(x == 2 for x in r[0]) and c["env"].get("CLRSDP_SCHUR_GRP2") != "0"


def _stage(pk, c, inst, lu_sq=False):
    """Decoy state, then the case's state, on one handle: (info before, info after, X^-1, S, A_Y)."""
    from clrsdp_amd import _lib as L
    cons, b, bi, st, dec = inst
    w = c["words"]
    exact = w > 1
    P = pk.make_params("0.3", "0.1", "0.7", 0)
    dev = pk.DeviceSolver(cons, b, bi, precision_words=w)
    try:
        if lu_sq:
            dev.set_factorization(L.FACT_FALLBACK | L.FACT_LU_SQ)
        before = dev.schur_info()
        for state in (dec, st):
            dev.set_state(*state)
            for stage in (L.STAGE_MU_R, L.STAGE_XINV, L.STAGE_SCHUR):
                dev.run_stage(stage, P, False)
        info = dev.schur_info()
        get = lambda k: np.array(dev.buffer(k, exact), dtype=object if exact else float)
        return before, info, get(L.BUF_XINV), get(L.BUF_S), get(L.BUF_AY)
    finally:
        dev.close()


def _reference(key, inst, Xi_flat, words, klass):
    """(S, A_Y, bS, bA, how) from the device's own X^-1, computed once per (case, class, X^-1)."""
    from clrsdp_amd import instance as I
    cons, b, bi, st, dec = inst
    raw = Xi_flat.tobytes() if Xi_flat.dtype != object else repr(list(Xi_flat)).encode()
    key = key + (hash(raw),)
    if key not in _REF:
        _REF.clear()  # (one case at a time: the next test has another instance)
        Xi = I.flat_to_blocks(Xi_flat, bi)
        _REF[key] = sc.reference_auto(cons, bi, Xi, st[3], words, klass)
    return _REF[key]


def _ratio(got, ref, bound):
    """schur_cases.cw_ratio, vectorised where the device's side is float64."""
    got = np.asarray(got)
    if got.dtype == object:
        return sc.cw_ratio(got, ref, bound)
    ref = np.asarray(ref)
    if ref.dtype == object:
        hi = np.array([float(v) for v in ref])
        lo = np.array([float(v - h) for v, h in zip(ref, hi)])
    else:
        hi = ref.astype(np.float64)
        lo = (ref - hi).astype(np.float64)
    if not np.isfinite(got).all():
        return np.inf
    d = np.abs((got - hi) - lo)
    bd = np.asarray(bound, dtype=float)
    if ((bd <= 0) & (d > 0)).any():
        return np.inf
    nz = d > 0
    return float((d[nz] / bd[nz]).max()) if nz.any() else 0.0


def _limbs_equal(got, ref):
    if np.asarray(got).dtype == object:
        return all(x == y for x, y in zip(got, ref))
    return all(float(y) == x for x, y in zip(got, ref)) if np.asarray(ref).dtype == object else \
        bool(np.array_equal(got, np.asarray(ref, dtype=np.float64)))


def _compare(c, klass, inst, out, tag):
    """Assert one run against the reference; returns (ratio S, ratio A_Y, bitwise, S)."""
    cons, b, bi, st, dec = inst
    before, info, Xi, S, AY = out
    w = c["words"]
    S_ref, AY_ref, bS, bA, how, bits = _reference((c["id"], klass), inst, Xi, w, klass)
    tS, tA = sc.tolerances(cons, bi, w)
    rS, rA = _ratio(S, S_ref, bS * tS), _ratio(AY, AY_ref, bA * tA)
    same = _limbs_equal(S, S_ref) and _limbs_equal(AY, AY_ref)
    print(f"SCHUR {c['row']} words={w} class={klass} {tag} id={c['id']} ref={how} bits={bits} "
          f"S={rS:.3g} A_Y={rA:.3g} equal={int(same)}")
    assert rS <= 1 and rA <= 1, (c["id"], klass, tag, rS, rA)
    if klass == "exact53":
        assert sc.fits_word(bits, w), (c["id"], bits)
    if klass in ("exact", "exact53") and sc.fits_word(bits, w):
        covered = True
        if info["ozaki"]:
            # the int8 products are exact where their sixteen digits cover the operands and no
            # digit product falls below the last level kept (schur_cases.ozaki_covers, derived
            # from the plan): that has to hold on exact53, and equality is asserted where it does
            from clrsdp_amd import instance as I
            covered = sc.ozaki_covers(cons, bi, I.flat_to_blocks(Xi, bi), st[3])
            assert covered or klass != "exact53", (c["id"], "the int8 digits do not cover exact53")
        if covered:
            assert same, (c["id"], klass, tag, "not equal in every limb", rS, rA)
    return rS, rA, same, S


def _instances(pk, c):
    w = c["words"]
    return (("random", sc.random_instance(pk, c["specs"], w)),
            ("exact", sc.exact_instance(pk, c["specs"], w)),
            ("exact53", sc.exact_instance(pk, c["specs"], w, small=True)))


def _set_env(monkeypatch, env):
    for k in sc.ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_info(c, info, before, extra=None):
    assert before["full"] == -1 and before["s_lower"] == -1, before
    want = dict(c["expect"], **(extra or {}))
    bad = {k: (info[k], v) for k, v in want.items() if info[k] != v}
    assert not bad, f"{c['id']}: schur_info (got, expected) {bad}; all of it: {info}"
    if info["one"]:
        assert info["n_fwg"] > 0
    if not info["fused"]:
        assert info["n_fwg"] == 0 and not info["one"] and not info["d64"] and not info["fused_y"]


FP64 = sc.fp64_cases()


@pytest.mark.parametrize("c", FP64, ids=[c["id"] for c in FP64])
def test_schur_fp64_dispatch_rows(pk, monkeypatch, c):
    """fp64, m = 1: one case of one row of the dispatch table (schur_cases.fp64_cases), on the
    random, exact and exact53 classes.  With the default flags full and s_lower are asserted as
    the row implies them (fused, every dim_S <= 256, no schur_gsum cluster: full = 0, the kernel
    stores the lower triangle and the upper one read here is the host's mirror; without the fused
    kernel full = 1 always); the dagger rows run again with
    FACT_LU_SQ: full = 1, s_lower = 0, both raw triangles against the reference, bitwise mirrors
    where S_j is written directly."""
    _set_env(monkeypatch, c["env"])
    for klass, inst in _instances(pk, c):
        bi = inst[2]
        out = _stage(pk, c, inst)
        full = int(max(bi.dim_S) > 256 or out[1]["n_gsum"] > 0 or not out[1]["fused"])
        _assert_info(c, out[1], out[0], dict(full=c["expect"].get("full", full),
                                              s_lower=int(bool(out[1]["fused"]) and not full)))
        _compare(c, klass, inst, out, "default")
        if c["dagger"]:
            out = _stage(pk, c, inst, lu_sq=True)
            _assert_info(c, out[1], out[0], dict(full=1, s_lower=0))
            S = _compare(c, klass, inst, out, "lu_sq")[3]
            off = 0
            for j, D in enumerate(bi.dim_S):
                blk = S[off:off + D * D].reshape(D, D)
                if _direct(c, j):
                    assert np.array_equal(blk, blk.T), (c["id"], klass, j, "triangles differ")
                off += D * D


GENERAL = sc.general_cases()


@pytest.mark.parametrize("c", GENERAL, ids=[f"w{c['words']}-{c['id']}" for c in GENERAL])
def test_schur_general_path(pk, monkeypatch, c):
    """m > 1 at fp64, double-double and quad-double: four GEMMs, extract_AY and the 4-term
    schur_assemble; the int8 products report off because of anyMgt1.  Every entry of A_Y is
    compared in the reference's (l, r, s <= r, column) layout, which pins extract_AY's (r, s, p)
    order, and every entry of S_j, which includes the first and the last entry of every
    (rs1, rs2) panel of schur_assemble's tuple decode.  The kernel writes (p, q) and (q, p) from
    one value: both triangles of the raw BUF_S are bitwise mirrors."""
    _set_env(monkeypatch, c["env"])
    for klass, inst in _instances(pk, c):
        bi = inst[2]
        out = _stage(pk, c, inst)
        _assert_info(c, out[1], out[0])
        S = _compare(c, klass, inst, out, "default")[3]
        off = 0
        for j, D in enumerate(bi.dim_S):
            blk = S[off:off + D * D].reshape(D, D)
            assert all(blk[p, q] == blk[q, p] for p in range(D) for q in range(p)), (c["id"], klass, j)
            off += D * D


MW = sc.mw_cases()


def _pair_upper_runs(pk, monkeypatch, c, klass, inst):
    """The case with the upper-tile form of BX, BY on and off: each against the reference; whether
    the two are bitwise equal is printed, not asserted."""
    res = {}
    for pu in (1, 0):
        _set_env(monkeypatch, dict(c["env"], **({} if pu else {"CLRSDP_MW_PAIR_UPPER": "0"})))
        out = _stage(pk, c, inst)
        _assert_info(c, out[1], out[0], dict(pair_upper=pu))
        res[pu] = (_compare(c, klass, inst, out, f"pair_upper={pu}"), out[4])
    (S1, A1), (S0, A0) = ((res[p][0][3], res[p][1]) for p in (1, 0))
    same = all(x == y for x, y in zip(S1, S0)) and all(x == y for x, y in zip(A1, A0))
    print(f"SCHUR {c['row']} class={klass} id={c['id']} pair_upper on/off bitwise equal: {int(same)}")


@pytest.mark.parametrize("c", MW, ids=[c["id"] for c in MW])
def test_schur_multiword_m1(pk, monkeypatch, c):
    """Multi-word, m = 1: the int8 products (double-double default: ozaki = 1), the VALU products
    (CLRSDP_OZAKI=0, and quad-double), each with CLRSDP_MW_PAIR_UPPER on and off, at the 16-tile
    edges of oz_gemm and the `upper` tile list, its 64-wide k-chunks and oz_split's strides.
    With pair_upper on and off both results hold the bound (whether they are bitwise equal is
    printed: they need not be, the off form sums BX[p, q] BY[q, p], the on form (min, max))."""
    for klass, inst in _instances(pk, c):
        _pair_upper_runs(pk, monkeypatch, c, klass, inst)


GRADED = [(w, oz, g) for w, oz in ((2, 1), (2, 0), (4, 0)) for g in sc.GRADED]


@pytest.mark.parametrize("words,oz,shape", GRADED,
                         ids=[f"w{w}{'-oz' if oz else ''}-d{g[0]}r{g[1]}g{g[3]}" for w, oz, g in GRADED])
def test_schur_multiword_graded(pk, monkeypatch, words, oz, shape):
    """The graded class (helpers.graded_instance, the four shapes of
    test_schur_products_componentwise_on_graded_data) under the decoy rule, with the path
    asserted and pair_upper on and off; it holds on the int8 products too."""
    delta, rank, N, g = shape
    c = sc.case(f"graded{words}{'-oz' if oz else ''}", sc._one(delta, N, rank),
                {} if (oz or words == 4) else {"CLRSDP_OZAKI": "0"},
                dict(fast=0, fused=0, ozaki=oz, full=1, s_lower=0), words=words)
    c["id"] += f"g{g}"
    _pair_upper_runs(pk, monkeypatch, c, "graded", sc.graded(pk, delta, rank, N, g, words))
