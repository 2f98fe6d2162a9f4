"""The SCHUR stage on every row of its dispatch table: the exact reference of whole instances, the
componentwise bound, the operand classes and the case tables shared by tests/test_schur_host.py
(no GPU) and tests/test_gpu_schur.py.

Reference
    :func:`schur_reference` generalises helpers.schur_exact (one cluster, m = 1, L = 1) to what
    the stage computes: several clusters, L >= 1 blocks of different delta, m >= 1 (the 4-term
    formula with its factor 1/4, MPMP.jl:1373-1398, as helpers.schur_dense lays it out) and
    per-sample ranks including 0.  Every operand is a dyadic rational -- V, lambda and Y are
    float64 or limb sums, X^-1 is the device's own BUF_XINV read back exactly -- so every product
    and sum is done on Python integers with a shared power-of-two exponent and rounded once to
    320-bit mpmath; 1/4 is an exponent.  It also returns the componentwise scales bS, bA: the same
    formulas with every factor replaced by its absolute value (float64).

    fp64 cases with more than EXACT_K_MAX = 200 columns in a block, or with delta K (delta + K)
    above EXACT_COST_MAX = 4e6 in a block (delta = 128 from K = 129 on: the integer products take
    2.4 s at delta = 128, K = 193), take helpers.schur_dense instead (np.longdouble GEMMs, the
    same X^-1, the same bS): the integer products would take too long there for a test.  Its
    error is about (delta + T) 2^-64 bS, below 2^-9 of the fp64 bound 8 (delta + 2) 2^-53 bS.
    Multi-word cases always use the exact form and keep K <= 130.

Bound (componentwise, u = 2^-53 / 2^-104 / 2^-206 as in the product tests)
    |S - S_ref|     <= (8 (delta_max + 2) + 2 T) u bS
    |A_Y - A_Y_ref| <=  8 (delta_max + 2)        u bA
    delta_max: the largest delta of the cluster's blocks; T: the largest number of terms summed
    into one entry, max over (k1, k2) of sum_l rho_l,k1 rho_l,k2, times 4 at m > 1.
    Each term is a product of two factors (BX and BY entries); each factor is two chained
    length-delta dot products (gamma_delta each), then the lambda products and the Hadamard
    product: 4 (delta + 2) u to first order.  The sum of T terms adds (T - 1) u.  A factor 2 of
    slack.  At T = 1 this is the bound of test_schur_products_componentwise_on_graded_data.
    tests/test_schur_host.py shows that a plain float64 NumPy restatement stays below it on every
    fp64 case of the tables (so it is not fitted to the device) and that it is sharp (dropped
    terms, stale tiles, wrong factors all exceed it).

Operand classes
    random   synth_mixed's V, lambda; SPD X, Y from rand_spd.  Multi-word: every limb of X, Y, V
             and lambda filled (:func:`fill_limbs`: limbs that cannot overlap, so the limb split
             of to_planes hands the device exactly the value the reference takes).
    graded   helpers.graded_instance (single block), as test_gpu_parity.py has it.
    exact    V integers in [-3, 3] times 2^-(i mod 8), lambda in {1/2, 1, 2}, X = diag(4^(i mod 5))
             (its Cholesky factor and inverse are exact), Y integer symmetric with |offdiag| <= 3
             and diagonal 4 delta (diagonally dominant, SPD); multi-word cases add a second
             integer at 2^-70 to V.
             Where every intermediate fits the word, S and A_Y must equal the reference in every
             limb whatever the order of summation; :func:`fits_word` decides that from the
             integers themselves (every sum of absolute values, in units of the smallest bit that
             occurs, below 2^53 / 2^104 / 2^206).  With the gradings above the products
             BX o BY span about 70 bits (V V: 14 + 4, X^-1: 8, the delta-sums: 2 x 8, Y: 10, ...),
             so at fp64 that holds only for the smallest delta, and with the 2^-70 term not at
             double-double either; where it does not hold the exact class is held to the
             componentwise bound like the random one (its sums have no cancellation to hide a
             dropped term).
    exact53  the same construction with the gradings cut to 2^-(i mod 2) and 4^(i mod 2) and
             |offdiag Y| <= 1, so that at fp64 every intermediate fits 53 bits at every shape of
             the tables (at most 40 are needed): equal in every limb on every path.  V enters
             every entry of S four times, so a second integer at 2^-70 spans 280 bits and fits no
             word; the multi-word cases of this class put it at 2^-14 (double-double) and 2^-36
             (quad-double), which keeps every intermediate within 104 / 206 bits while the
             products still fill the lower limbs.  This is the check that catches a dropped
             k-term or tile outright.  On the int8 products (oz_split / oz_gemm) equality needs
             more than the word: the sixteen base-2^7 digits of every vector have to cover it and
             no digit product may fall below the last level kept.  :func:`ozaki_covers` derives
             that from the plan; it holds on every exact53 case, where equality is then asserted.
"""
import math

import numpy as np

from helpers import _exact_ints as _exact_ints_mp, _sample_sums, rand_spd, schur_dense

U = {1: 2.0 ** -53, 2: 2.0 ** -104, 4: 2.0 ** -206}
WORD_BITS = {1: 53, 2: 104, 4: 206}
EXACT_K_MAX = 200
EXACT_COST_MAX = 4e6   # delta K (delta + K) of a block: about 0.6 s of integer products
PREC = 320


# ---- operands ---------------------------------------------------------------------------------
def _exact_ints(a):
    """helpers._exact_ints (a = I 2^e exactly, I Python integers, e the smallest bit that occurs
    or 0), without the per-entry mpmath conversion when ``a`` is a float64 array."""
    a = np.asarray(a)
    if a.dtype == object:
        return _exact_ints_mp(a)
    a = a.astype(np.float64)
    assert np.isfinite(a).all()
    mant, ex = np.frexp(a)
    mi = np.ldexp(mant, 53).astype(np.int64)          # |mi| < 2^53, a = mi 2^(ex - 53)
    ex = ex.astype(np.int64) - 53
    nz = mi != 0
    low = mi & -mi                                        # the lowest set bit
    tz = np.zeros(a.shape, dtype=np.int64)
    tz[nz] = np.round(np.log2(low[nz].astype(np.float64))).astype(np.int64)
    e = min(int((ex + tz)[nz].min()), 0) if nz.any() else 0
    out = np.empty(a.size, dtype=object)
    for i, (m_, x_) in enumerate(zip(mi.ravel().tolist(), ex.ravel().tolist())):
        out[i] = (m_ << (x_ - e)) if x_ >= e else (m_ >> (e - x_))
    return out.reshape(a.shape), e


def _block_ops(cl, l):
    """(V delta x K, lam K, counts N, starts N) of block l of a cluster; V and lam float64, or
    object arrays of mpmath.mpf when the cluster holds multi-word values."""
    cols = [np.asarray(v) for vk in cl.A[l] for v in vk]
    counts = np.array([len(vk) for vk in cl.A[l]], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    lam = [x for hk in cl.H[l] for x in hk]
    if not cols:
        return None, None, counts, starts
    V = np.stack(cols, axis=1)
    lam = np.array(lam, dtype=object if V.dtype == object else float)
    return V, lam, counts, starts


def _absf(M):
    M = np.asarray(M)
    if M.dtype != object:
        return np.abs(M.astype(float))
    return np.abs(np.array([float(v) for v in M.ravel()]).reshape(M.shape))


def _shift_add(acc, e_acc, add, e_add):
    """(acc 2^e_acc + add 2^e_add) as (integers, exponent); acc None = zero."""
    if acc is None:
        return add, e_add
    e = min(e_acc, e_add)
    return acc * (1 << (e_acc - e)) + add * (1 << (e_add - e)), e


def _mirror_upper(M):
    """Symmetric(M) from its upper triangle (MPMP.jl:1409), in place."""
    iu = np.triu_indices(len(M), 1)
    M[(iu[1], iu[0])] = M[iu]
    return M


def _to_mpf(ints, e, prec):
    import mpmath
    with mpmath.workprec(prec):
        return np.array([mpmath.ldexp(mpmath.mpf(int(v)), e) for v in ints], dtype=object)


def terms_per_entry(cl, m):
    """T of the bound: the largest number of products summed into one entry of S_j."""
    C = np.array([[len(vk) for vk in Al] for Al in cl.A], dtype=np.int64)
    return int((C.T @ C).max()) * (4 if m > 1 else 1)


def schur_reference(cons, bi, X_inv, Y, prec=PREC, mut=None):
    """S and A_Y of a whole instance in the layout of BUF_S and BUF_AY (flat object arrays of
    mpmath.mpf rounded once to ``prec`` bits) from X_inv[j][l] and Y[j][l] (float64 or mpf
    entries), with the componentwise scales bS, bA (flat float64).

    ``mut`` names one deliberate mistake for the sharpness test of tests/test_schur_host.py
    (``{"drop_k": i}``: contraction index i of the first block left out of V^T X^-1 V and
    V^T Y V; ``{"lam": c}``: the row-side lambda of column c taken as 1; ``{"quarter": 1}``: the
    1/4 left out at m > 1; ``{"group_term": 1}``: one term of the first sample group of more than
    one column left out; ``{"by_untransposed": 1}``: BY blocks taken untransposed at m > 1)."""
    mut = mut or {}
    S_out, AY_out, bS_out, bA_out = [], [], [], []
    for j in range(bi.J):
        m, N, D = bi.m[j], bi.n_samples[j], bi.dim_S[j]
        cl = cons[j]
        Sj, eS = None, 0
        bSj = np.zeros((D, D))
        for l in range(bi.L[j]):
            V, lam, counts, starts = _block_ops(cl, l)
            if V is None:
                continue
            delta, K = V.shape
            Vi, ev = _exact_ints(V)
            Xi, ex = _exact_ints(X_inv[j][l])
            Yi, ey = _exact_ints(Y[j][l])
            li, el = _exact_ints(lam)
            Vc = Vi
            if "drop_k" in mut and l == 0 and j == 0:
                Vc = Vi.copy()
                Vc[mut["drop_k"], :] = 0
            blk = lambda M, r, s: M[r * delta:(r + 1) * delta, s * delta:(s + 1) * delta]
            BX = [[Vi.T @ (blk(Xi, r, s) @ Vc) for s in range(m)] for r in range(m)]
            BY = [[Vi.T @ (blk(Yi, r, s) @ Vc) for s in range(m)] for r in range(m)]
            aV, aX, aY, al = _absf(V), _absf(X_inv[j][l]), _absf(Y[j][l]), _absf(lam)
            bX = [[aV.T @ blk(aX, r, s) @ aV for s in range(m)] for r in range(m)]
            bY = [[aV.T @ blk(aY, r, s) @ aV for s in range(m)] for r in range(m)]
            AY_out.append(_to_mpf(np.concatenate([np.diagonal(BY[r][s]) for r in range(m)
                                                  for s in range(r + 1)]), 2 * ev + ey, prec))
            bA_out += [np.diagonal(bY[r][s]).copy() for r in range(m) for s in range(r + 1)]
            lrow = li.copy()
            if "lam" in mut and l == 0 and j == 0:
                lrow[mut["lam"]] = 1 << (-el)
            LL, aLL = np.outer(lrow, li), np.outer(al, al)
            tr = (lambda M: M) if mut.get("by_untransposed") else (lambda M: M.T)
            Sl = np.zeros((D, D), dtype=object)
            for r1 in range(m):
                for s1 in range(r1 + 1):
                    for r2 in range(m):
                        for s2 in range(r2 + 1):
                            if m == 1:
                                T, bT = BX[0][0] * BY[0][0].T, bX[0][0] * bY[0][0].T
                            else:
                                T = (BX[s1][r2] * tr(BY[s2][r1]) + BX[r1][r2] * tr(BY[s2][s1])
                                     + BX[s1][s2] * tr(BY[r2][r1]) + BX[r1][s2] * tr(BY[r2][s1]))
                                bT = (bX[s1][r2] * bY[s2][r1].T + bX[r1][r2] * bY[s2][s1].T
                                      + bX[s1][s2] * bY[r2][r1].T + bX[r1][s2] * bY[r2][s1].T) / 4
                            G = LL * T
                            if mut.get("group_term") and l == 0 and j == 0 and r1 == s1 == r2 == s2 == 0:
                                k = int(np.argmax(counts > 1))
                                G[starts[k] + 1, starts[k]] = 0
                            h0 = (s1 + r1 * (r1 + 1) // 2) * N
                            v0 = (s2 + r2 * (r2 + 1) // 2) * N
                            Sl[v0:v0 + N, h0:h0 + N] += _sample_sums(G, starts, counts).T
                            bSj[v0:v0 + N, h0:h0 + N] += _sample_sums(aLL * bT, starts, counts).T
            e_l = 2 * el + 4 * ev + ex + ey - (2 if m > 1 and not mut.get("quarter") else 0)
            Sj, eS = _shift_add(Sj, eS, Sl, e_l)
        if Sj is None:
            Sj = np.zeros((D, D), dtype=object)
        _mirror_upper(Sj)
        _mirror_upper(bSj)
        S_out.append(_to_mpf(Sj.reshape(-1, order="F"), eS, prec))
        bS_out.append(bSj.reshape(-1, order="F"))
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dtype=dt)
    return cat(S_out, object), cat(AY_out, object), cat(bS_out, float), cat(bA_out, float)


def span_bits(cons, bi, X_inv, Y):
    """An upper bound of the bit span of every intermediate of the stage: each block's operands
    are integers in units of their smallest bit (2^ev, 2^ex, 2^ey, 2^el), and no partial sum, in
    any order, exceeds the same sum on absolute values.  The largest of those -- |V|^T |X^-1| |V|,
    |V|^T |Y| |V| over the whole m delta block, and T_max lambda_max^2 times their product -- in
    units of 2^(2 el + 4 ev + ex + ey), as a bit count (float64 arithmetic, one bit of margin)."""
    bits = 0
    for j in range(bi.J):
        m = bi.m[j]
        T = terms_per_entry(cons[j], m)
        for l in range(bi.L[j]):
            V, lam, counts, starts = _block_ops(cons[j], l)
            if V is None:
                continue
            ev, ex, ey, el = (_exact_ints(a)[1] for a in (V, X_inv[j][l], Y[j][l], lam))
            aV = np.kron(np.ones((m, 1)), _absf(V))
            # in log2: the units of a random quad-double case are about 2^-800
            lg = lambda v: math.log2(v) if v > 0 else -math.inf
            sx = lg(float((aV.T @ _absf(X_inv[j][l]) @ aV).max())) - (2 * ev + ex)
            sy = lg(float((aV.T @ _absf(Y[j][l]) @ aV).max())) - (2 * ev + ey)
            sl = lg(float(_absf(lam).max())) - el
            bits = max(bits, int(math.ceil(max(sx + sy + 2 * sl + lg(T), sx, sy, 0.0))) + 1)
    return bits


def fits_word(bits, words):
    """Every intermediate of the stage is an integer below 2^bits in units of the smallest bit
    that occurs, so it is exact in the word whatever the order of summation.  (Conservative for
    the multi-word formats, whose limbs need not be contiguous.)"""
    return bits <= WORD_BITS[words]


OZ_DIGITS, OZ_BASE_BITS = 16, 7   # oz_split: OZ_S digits of base 2^7 per element (kernels_dense.h)


def _digits_needed(M, eq, axis):
    """For every vector of the integer matrix M (vectors along ``axis``), element k scaled by
    2^eq[k]: the number P of base-2^7 digits after which oz_split's remainder is zero.  The split
    scales the vector by 2^-E, E = (largest exponent) + 2, and digit p carries the bits down to
    2^(E - 7 (p + 1)), so P = ceil((E - lowest set bit) / 7); one bit more is allowed for, since
    the kernel takes the exponent from the leading limb, which may round up to a power of two."""
    M = np.asarray(M, dtype=object)
    M = M if axis == 1 else M.T
    worst = 0
    for vec in M:
        top = [int(v).bit_length() - 1 + e for v, e in zip(vec, eq) if v]
        low = [(int(v) & -int(v)).bit_length() - 1 + e for v, e in zip(vec, eq) if v]
        if top:
            worst = max(worst, -(-(max(top) + 3 - min(low)) // OZ_BASE_BITS))
    return worst


def ozaki_covers(cons, bi, X_inv, Y):
    """Whether the int8 products of a double-double m = 1 instance are exact, from the plan
    (Solver::build_ozaki, oz_split, oz_gemm): per block the four products X^-1 V, Y V, V^T (X^-1 V),
    V^T (Y V), the contraction index k scaled by 2^(+-kx[k]), kx[k] the exponent of the largest
    |V_k.|.  A product of a row needing P_a digits with a column needing P_b is exact when
      * P_a, P_b <= 16 (the split leaves no remainder), and
      * P_a + P_b <= 17 (digit products d_p g_q with p + q >= 16 are the levels oz_gemm drops;
        digits p >= P_a and q >= P_b are zero, so none is dropped), and
      * the result fits: the levels are summed by two_sum into hi with the errors added into lo in
        plain fp64, sixteen of them, each at most half an ulp of hi: lo is exact while
        16 * 2^(bits - 53) / 2 < 2^53, that is span_bits <= 102 (the same bound lets TX, TY, BX,
        BY sit in a double-double exactly).
    Every level's int32 sum is exact by construction (Kpad < 2^15)."""
    if span_bits(cons, bi, X_inv, Y) > 102:
        return False
    for j in range(bi.J):
        for l in range(bi.L[j]):
            V, lam, counts, starts = _block_ops(cons[j], l)
            if V is None:
                continue
            Vi, ev = _exact_ints(V)
            Xi, ex = _exact_ints(X_inv[j][l])
            Yi, ey = _exact_ints(Y[j][l])
            hi = _absf(V).max(axis=1)
            kx = [int(math.frexp(h)[1]) - 1 if h > 0 else 0 for h in hi]
            neg = [-e for e in kx]
            Pv = _digits_needed(Vi, neg, 0)                 # columns of V, k scaled by 2^-kx
            for M in (Xi, Yi):
                Pm = _digits_needed(M, kx, 1)               # rows of X^-1 / Y, k scaled by 2^+kx
                Pt = _digits_needed(M @ Vi, kx, 0)          # columns of TX / TY, k scaled by 2^+kx
                if max(Pv, Pm, Pt) > OZ_DIGITS or Pm + Pv > OZ_DIGITS + 1 or Pv + Pt > OZ_DIGITS + 1:
                    return False
    return True


def schur_longdouble(cons, bi, X_inv, Y):
    """The fp64 reference above EXACT_K_MAX: helpers.schur_dense (np.longdouble GEMMs, error
    about (delta + T) 2^-64 bS, below 2^-9 of the fp64 bound) with the scales of
    :func:`scales_only`."""
    S, AY = schur_dense(cons, bi, X_inv, Y)
    bS, bA = scales_only(cons, bi, X_inv, Y)
    return S, AY, bS, bA


def scales_only(cons, bi, X_inv, Y):
    """bS, bA alone: schur_dense on absolute values, in float64."""
    import copy
    ac = [copy.copy(cl) for cl in cons]
    for cl in ac:
        cl.A = [[[_absf(v) for v in vk] for vk in Al] for Al in cl.A]
        cl.H = [[[abs(float(x)) for x in hk] for hk in Hl] for Hl in cl.H]
    aX = [[_absf(M) for M in Xj] for Xj in X_inv]
    aY = [[_absf(M) for M in Yj] for Yj in Y]
    bS, bA = schur_dense(ac, bi, aX, aY, dtype=np.float64)
    return bS, bA


def reference_auto(cons, bi, X_inv, Y, words, klass, ints=True):
    """(S, A_Y, bS, bA, how, bits): the reference a case is held to.  The exact classes at fp64
    whose intermediates fit 53 bits are exact in plain float64 ("f64-exact"), those that fit 64
    bits in np.longdouble ("ld-exact"); fp64 cases with more than EXACT_K_MAX columns in a block
    or delta K (delta + K) above EXACT_COST_MAX take the longdouble GEMMs ("ld"); everything
    else, and every multi-word case, the integer form ("int").  ``ints`` False: "ld" for every
    fp64 case (the host test of the float64 restatement, which measures ratios near 0.1)."""
    Kmax = max(rs[-1] for rj in bi.rank_sums for rs in rj)
    cost = max((n // bi.m[j]) * rs[-1] * (n // bi.m[j] + rs[-1]) * bi.m[j] ** 2
               for j, rj in enumerate(bi.rank_sums) for n, rs in zip(bi.Y_blocksizes[j], rj))
    bits = span_bits(cons, bi, X_inv, Y)
    if words == 1 and klass in ("exact", "exact53") and bits <= 53:
        S, AY = schur_float64(cons, bi, X_inv, Y)
        bS, bA = scales_only(cons, bi, X_inv, Y)
        how = "f64-exact"
    elif words == 1 and klass in ("exact", "exact53") and bits <= 64 and np.finfo(np.longdouble).nmant >= 63:
        S, AY, bS, bA = schur_longdouble(cons, bi, X_inv, Y)
        how = "ld-exact"
    elif words == 1 and (Kmax > EXACT_K_MAX or cost > EXACT_COST_MAX or not ints):
        S, AY, bS, bA = schur_longdouble(cons, bi, X_inv, Y)
        how = "ld"
    else:
        S, AY, bS, bA = schur_reference(cons, bi, X_inv, Y)
        how = "int"
    return S, AY, bS, bA, how, bits


def schur_float64(cons, bi, X_inv, Y):
    """The plain NumPy float64 restatement (float64 GEMMs, Hadamard products, _sample_sums): what
    a straightforward fp64 implementation of the formula gives.  (S, A_Y), flat float64."""
    return schur_dense(cons, bi, X_inv, Y, dtype=np.float64)


def tolerances(cons, bi, words):
    """Per entry of BUF_S and BUF_AY the factor of the bound: (8 (delta_max + 2) + 2 T) u and
    8 (delta_max + 2) u of the entry's cluster."""
    u = U[words]
    tS, tA = [], []
    for j in range(bi.J):
        m = bi.m[j]
        dmax = max(n // m for n in bi.Y_blocksizes[j])
        T = terms_per_entry(cons[j], m)
        tS.append(np.full(bi.dim_S[j] ** 2, (8 * (dmax + 2) + 2 * T) * u))
        for l in range(bi.L[j]):
            tA.append(np.full(m * (m + 1) // 2 * bi.rank_sums[j][l][-1], 8 * (dmax + 2) * u))
    return np.concatenate(tS), np.concatenate(tA) if tA else np.zeros(0)


def cw_ratio(got, ref, bound):
    """max over entries of |got - ref| / bound (``bound`` > 0 per entry, or 0 where the reference
    is an exact zero that must be reproduced), at 320 bits.  A non-finite entry gives inf."""
    import mpmath
    g, r = np.asarray(got, dtype=object).ravel(), np.asarray(ref, dtype=object).ravel()
    bd = np.asarray(bound, dtype=float).ravel()
    assert len(g) == len(r) == len(bd), (len(g), len(r), len(bd))
    worst = 0.0
    with mpmath.workprec(320):
        for x, y, s in zip(g, r, bd):
            d = abs(mpmath.mpf(x) - mpmath.mpf(y))
            if not mpmath.isfinite(d):
                return math.inf
            if d == 0:
                continue
            worst = max(worst, float(d / mpmath.mpf(s))) if s > 0 else math.inf
    return worst


# ---- instances ----------------------------------------------------------------------------------
def sp(m, deltas, N, ranks=None):
    return dict(m=m, deltas=list(deltas), N=N, ranks=ranks)


def ranks_of(kind, L, N):
    """Per-sample ranks: 1, 2 (all), or "cyc": (k + 3 + 2 l) mod 4 in block l -- cycling 3, 0, 1,
    2 (so that N = 1 has vectors, three of them: a group sum), and at L = 2 no sample has rank 0
    in both blocks.  At L = 1
    every fourth sample has no vector at all: its row and column of S_j are zero and have to be
    written as such."""
    if kind == 1:
        return None
    if kind == 2:
        return [[2] * N for _ in range(L)]
    assert kind == "cyc"
    return [[(k + 3 + 2 * l) % 4 for k in range(N)] for l in range(L)]


def fill_limbs(a, words, rng, sym=False):
    """float64 array -> object array of mpmath.mpf with every one of the ``words`` limbs filled:
    a + sum_q fl(a e_q) 2^(-55 q), |e_q| uniform in [1/4, 1/2) with a random sign (a symmetric
    array of them when ``sym``), summed exactly.  Limb q + 1 is below 2^-54 of limb q, less than
    half an ulp of it, so the limbs cannot overlap and to_planes' split (each limb the nearest
    double of what is left) returns exactly these limbs: the device receives this value."""
    import mpmath
    a = np.asarray(a, dtype=float)
    if words == 1:
        return a
    limbs = [a]
    for q in range(1, words):
        e = rng.uniform(0.25, 0.5, size=a.shape) * rng.choice([-1.0, 1.0], size=a.shape)
        if sym:
            e = np.triu(e) + np.triu(e, 1).T
        limbs.append(np.ldexp(limbs[0] * e, -55 * q))
    out = np.empty(a.size, dtype=object)
    for i, vs in enumerate(zip(*[p.ravel() for p in limbs])):
        acc = mpmath.mpf(float(vs[0]))
        for v in vs[1:]:
            acc = mpmath.fadd(acc, float(v), exact=True)
        out[i] = acc
    return out.reshape(a.shape)


def _state(bi, seed, words, scale=1.0):
    rng = np.random.default_rng(seed)
    sym = lambda M: (M + M.T) / 2
    X = [[fill_limbs(scale * sym(rand_spd(n, rng)), words, rng, True) for n in bj] for bj in bi.Y_blocksizes]
    Y = [[fill_limbs(scale * sym(rand_spd(n, rng)), words, rng, True) for n in bj] for bj in bi.Y_blocksizes]
    return np.zeros(sum(bi.dim_S)), X, np.zeros(bi.n_y), Y


def random_instance(pk, specs, words, seed=31):
    """(cons, b, bi, state, decoy state): synth_mixed's clusters (multi-word: every limb of V and
    lambda filled), an SPD state from rand_spd and the decoy of the stale-data rule -- the same
    instance with X, Y of another seed, scaled by 8 (float64 values at every width)."""
    cons, b = pk.synth_mixed(specs, 2, seed=seed)
    rng = np.random.default_rng(seed + 1)
    if words > 1:
        for cl in cons:
            cl.A = [[[fill_limbs(v, words, rng) for v in vk] for vk in Al] for Al in cl.A]
            cl.H = [[list(fill_limbs(np.array(hk, dtype=float), words, rng)) for hk in Hl] for Hl in cl.H]
    bi = pk.get_block_info(cons)
    return cons, b, bi, _state(bi, seed + 2, words), _state(bi, seed + 3, 1, 8.0)


def graded(pk, delta, rank, N, g, words, seed=21):
    """helpers.graded_instance with a decoy state (another seed's Mx, My on the same grading,
    scaled by 8)."""
    from helpers import graded_instance
    cons, b, st = graded_instance(pk, delta, rank, N, g, seed=seed)
    _, _, dec = graded_instance(pk, delta, rank, N, g, seed=seed + 1)
    dec = (dec[0], [[8.0 * dec[1][0][0]]], dec[2], [[8.0 * dec[3][0][0]]])
    return cons, b, pk.get_block_info(cons), st, dec


def exact_instance(pk, specs, words, seed=41, small=False):
    """The exact class (``small``: exact53) on the shapes of ``specs``; see the module docstring.
    The decoy state has X = 8 diag(4^((i + 2) mod 5)) and another integer Y, times 8."""
    import mpmath
    cons, b = pk.synth_mixed(specs, 2, seed=seed)
    rng = np.random.default_rng(seed)
    vm, xm, off = (2, 2, 1) if small else (8, 5, 3)
    low = -70 if not small else {1: 0, 2: -14, 4: -36}[words]
    for cl in cons:
        A, H = [], []
        for Al in cl.A:
            counts = [len(vk) for vk in Al]
            K, d = sum(counts), max(len(v) for vk in Al for v in vk)
            M = rng.integers(-3, 4, size=(K, d)).astype(float)
            M[~M.any(axis=1), 0] = 1.0
            M *= np.ldexp(1.0, -(np.arange(d) % vm))[None, :]
            lam = rng.choice([0.5, 1.0, 2.0], size=K)
            if words > 1:
                lo = rng.integers(-3, 4, size=(K, d))
                M = np.array([mpmath.fadd(float(a), mpmath.ldexp(mpmath.mpf(int(c)), low), exact=True)
                              for a, c in zip(M.ravel(), lo.ravel())], dtype=object).reshape(K, d)
                lam = [mpmath.mpf(float(v)) for v in lam]
            rows, lam = list(M), [v if words > 1 else float(v) for v in lam]
            Al2, Hl2, q = [], [], 0
            for n in counts:
                Al2.append(rows[q:q + n])
                Hl2.append(lam[q:q + n])
                q += n
            A.append(Al2)
            H.append(Hl2)
        cl.A, cl.H = A, H
    bi = pk.get_block_info(cons)

    def state(shift, scale):
        X, Y = [], []
        for bj in bi.Y_blocksizes:
            Xj, Yj = [], []
            for n in bj:
                Xj.append(scale * np.diag(4.0 ** ((np.arange(n) + shift) % xm)))
                M = np.triu(rng.integers(-off, off + 1, size=(n, n)).astype(float), 1)
                Yj.append(scale * (M + M.T + np.diag(np.full(n, 4.0 * n))))
            X.append(Xj)
            Y.append(Yj)
        return np.zeros(sum(bi.dim_S)), X, np.zeros(bi.n_y), Y
    return cons, b, bi, state(0, 1.0), state(2, 8.0)


# ---- the case tables ("The Schur stage on every dispatch row: tests") ------------
ENV_SWITCHES = ("CLRSDP_SCHUR_FUSED", "CLRSDP_SCHUR_FUSED_ONE", "CLRSDP_SCHUR_FUSED_D64",
                "CLRSDP_SCHUR_FUSED_Y", "CLRSDP_SCHUR_GRP2", "CLRSDP_OZAKI", "CLRSDP_MW_PAIR_UPPER")
K_FULL = (1, 63, 64, 65, 129, 192, 193, 257, 320)   # T = ceil(K / 64) in {1, 2, 3, 4, 5}
K_THIN = (1, 65, 193)
N_GRP2 = (1, 32, 33, 64, 65, 96, 97, 160)
MULTI = {"CLRSDP_SCHUR_FUSED": "1", "CLRSDP_SCHUR_FUSED_ONE": "0"}
UNFUSED = {"CLRSDP_SCHUR_FUSED": "0"}


def case(row, specs, env=None, expect=None, dagger=False, words=1):
    def tag(s):
        r = s["ranks"]
        rk = "r1" if r is None else ("r2" if all(x == 2 for rl in r for x in rl) else "rc")
        return f"m{s['m']}d{'_'.join(map(str, s['deltas']))}N{s['N']}{rk}"
    sw = "".join(f"-{k[7:].lower()}{v}" for k, v in sorted((env or {}).items()))
    return dict(row=row, specs=specs, env=dict(env or {}), expect=dict(expect or {}), dagger=dagger,
                words=words, id=f"{row}-" + "+".join(tag(s) for s in specs) + sw)


def _one(delta, N, rank):
    return [sp(1, [delta], N, ranks_of(rank, 1, N))]


def fp64_cases():
    """fp64, m = 1: every row of the dispatch table.  K = rho N columns per block,
    T = ceil(K / 64) row blocks.  The natural multi-tile choice (fwg >= 128) stays with
    test_c3_full_size_newton_identities."""
    F = dict(fast=1, fused=1, fused_y=1, n_gsum=0)
    out = []
    for d in (1, 3, 4, 5, 31, 32, 33, 63, 64):
        for K in (K_FULL if d in (33, 64) else K_THIN):
            out.append(case("one-d64", _one(d, K, 1), {}, dict(F, one=1, d64=1, grp2=0), True))
    for d in (5, 33, 64):
        for N in N_GRP2:
            out.append(case("one-d64-grp2", _one(d, N, 2), {}, dict(F, one=1, d64=1, grp2=1), True))
    for d in (65, 96, 97, 127, 128):
        for K in (K_FULL if d in (97, 128) else K_THIN):
            out.append(case("one-pad", _one(d, K, 1), {}, dict(F, one=1, d64=0, grp2=0), True))
    for d in (33, 64):
        for K in (65, 193):
            # (D64=0 alone sends delta <= 64 to the unfused pair: fused_one needs delta > 64 or
            # the D64 instance, so the ONE form is asked for as test_stage_parity_fp64_schur_paths'
            # "1-pad" does)
            out.append(case("one-pad-small", _one(d, K, 1),
                            {"CLRSDP_SCHUR_FUSED_D64": "0", "CLRSDP_SCHUR_FUSED_ONE": "1"},
                            dict(F, one=1, d64=0, grp2=0)))
    for d in (65, 128):
        for N in N_GRP2:
            out.append(case("one-grp2", _one(d, N, 2), {}, dict(F, one=1, d64=0, grp2=1), True))
    for d in (33, 64, 65, 128):
        for K in (64, 65, 193, 257, 320):
            out.append(case("multi", _one(d, K, 1), MULTI, dict(F, one=0, d64=0, grp2=0), True))
        for N in (33, 97, 160):
            out.append(case("multi-grp2", _one(d, N, 2), MULTI, dict(F, one=0, d64=0, grp2=1), True))
    ty = dict(MULTI, CLRSDP_SCHUR_FUSED_Y="0")
    for d in (65, 128):
        for K in (65, 193, 320):
            out.append(case("multi-ty", _one(d, K, 1), ty, dict(F, one=0, fused_y=0, grp2=0)))
        for N in (33, 97):
            out.append(case("multi-ty-grp2", _one(d, N, 2), ty, dict(F, one=0, fused_y=0, grp2=1)))
    P = dict(fast=1, fused=0, n_fwg=0, n_gsum=0)
    for d, env in [(129, {}), (150, {})] + [(d, UNFUSED) for d in (1, 16, 17, 64, 128)]:
        for K in (1, 63, 64, 65, 129, 193):
            out.append(case("pairs", _one(d, K, 1), env, dict(P, grp2=0), True))
        for N in (1, 33, 97):
            out.append(case("pairs-grp2", _one(d, N, 2), env, dict(P, grp2=1), True))
    for N in (1, 33, 65, 97):
        for env, fu in (({}, 1), (UNFUSED, 0)):
            G = dict(fast=1, n_gsum=1, grp2=0)
            for d2 in ((33, 20), (65, 128), (129, 40)):
                f = fu if max(d2) <= 128 else 0
                out.append(case("gsum-L2", [sp(1, d2, N)], env, dict(G, fused=f)))
            out.append(case("gsum-cyc", [sp(1, [40], N, ranks_of("cyc", 1, N))], env, dict(G, fused=fu)))
            out.append(case("gsum-nogrp2", _one(40, N, 2), dict(env, CLRSDP_SCHUR_GRP2="0"),
                            dict(G, fused=fu)))
    # mixed handles: the library's own choice, switches unset
    for N in (33, 65):
        out.append(case("mix-r2-r1", _one(40, N, 2) + _one(40, N, 1), {},
                        dict(fast=1, fused=0, grp2=1, n_gsum=0)))
        # delta 40 with delta 100 takes the unfused pair: below half the CUs the ONE form wants
        # every delta > 64 or the D64 instance, and D64 wants every delta <= 64 (the padded form
        # lost 2 % to the pair at delta = 64), so a handle on both sides of 64 has
        # neither
        out.append(case("mix-40-100", _one(40, N, 1) + _one(100, N, 1), {},
                        dict(fast=1, fused=0, grp2=0, n_gsum=0)))
        out.append(case("mix-100-140", _one(100, N, 1) + _one(140, N, 1), {},
                        dict(fast=1, fused=0, n_gsum=0)))
        out.append(case("mix-direct-L2", _one(40, N, 1) + [sp(1, (33, 20), N)], {},
                        dict(fast=1, fused=1, one=1, n_gsum=1, full=1)))
    out.append(case("dimS-257", _one(40, 257, 1), {}, dict(F, one=1, d64=1, full=1)))
    return out


def general_cases():
    """m > 1 (four GEMMs, extract_AY, the 4-term schur_assemble) at every width; Ozaki off
    because of anyMgt1.  The full product m x L x delta x N x ranks is 288 per width; kept are
    the corners delta, N in {1, 17} with every (m, L, ranks) at delta = N = 17, the tile edges
    (16, 16), (16, 17), (17, 16) at m = 2, L = 1, and delta = 7, N = 5 -- dropped: the interior
    combinations of (1, 5, 7) with the others."""
    out = []
    G = dict(fast=0, fused=0, ozaki=0, pair_upper=0, full=1, s_lower=0)
    for w in (1, 2, 4):
        for m in (2, 3):
            for L in (1, 2):
                for rk in (1, 2, "cyc"):
                    deltas = [17] if L == 1 else [17, 16]
                    out.append(case("general", [sp(m, deltas, 17, ranks_of(rk, L, 17))], {}, G, words=w))
        for d, N in ((1, 1), (1, 17), (17, 1), (16, 16), (16, 17), (17, 16), (7, 5)):
            out.append(case("general", [sp(2, [d], N)], {}, G, words=w))
        out.append(case("general-mix", [sp(2, [7], 16), sp(1, [16], 17)], {}, G, words=w))
    return out


def mw_cases():
    """Multi-word, m = 1: the int8 products (double-double default), the VALU products
    (CLRSDP_OZAKI=0; quad-double always), each with pair_upper on and off (paired in the test).
    delta and K run over the 16-tile and 64-chunk edges on a cross, not the full product (81 per
    column): every delta at K = 17 and K = 65, every K at delta = 17 and 65, and the corner
    (129, 129) -- dropped: the other combinations of two edge values."""
    out = []
    D = (1, 15, 16, 17, 63, 64, 65, 128, 129)
    Ks = (1, 15, 16, 17, 63, 64, 65, 129)
    cross = sorted({(d, K) for d in D for K in (17, 65)} | {(d, K) for d in (17, 65) for K in Ks}
                   | {(129, 129)})
    for w, oz in ((2, 1), (2, 0), (4, 0)):
        env = {} if (w == 4 or oz) else {"CLRSDP_OZAKI": "0"}
        E = dict(fast=0, fused=0, ozaki=oz, full=1, s_lower=0)
        for d, K in cross:
            out.append(case(f"mw{w}{'-oz' if oz else ''}", _one(d, K, 1), env, E, words=w))
        row = f"mw{w}{'-oz' if oz else ''}"
        for d, N in ((17, 33), (65, 17)):
            out.append(case(row, _one(d, N, 2), env, E, words=w))
            out.append(case(row, [sp(1, [d], N, ranks_of("cyc", 1, N))], env, E, words=w))
        out.append(case(row, [sp(1, (17, 16), 33, ranks_of("cyc", 2, 33))], env, E, words=w))
    return out


GRADED = [(12, 1, 23, 0), (12, 1, 23, 4), (40, 2, 79, 0), (40, 2, 79, 1)]
