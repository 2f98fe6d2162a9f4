"""Shared test helpers: instances, dense reconstructions of the constraint matrices, metrics."""
import math

import numpy as np


def dense_A(cl, bi, j, t_idx):
    """Dense block-diagonal (list over l) constraint matrix A_{j,(r,s,k)} (MPMP.jl:385-386)."""
    m, N = bi.m[j], bi.n_samples[j]
    loc = t_idx
    k = loc % N
    rs = loc // N
    r = 0
    while (r + 1) * (r + 2) // 2 <= rs:
        r += 1
    s = rs - r * (r + 1) // 2
    E = np.zeros((m, m))
    if r == s:
        E[r, r] = 1.0
    else:
        E[r, s] = E[s, r] = 0.5
    out = []
    for l in range(bi.L[j]):
        d = bi.Y_blocksizes[j][l] // m
        W = np.zeros((d, d))
        for v, lam in zip(cl.A[l][k], cl.H[l][k]):
            v = np.asarray(v, dtype=float)
            W += float(lam) * np.outer(v, v)
        out.append(np.kron(E, W))
    return out


def rand_spd(n, rng, shift=1.0):
    G = rng.standard_normal((n, n))
    return G @ G.T / n + shift * np.eye(n)


def rel_err(a, b, scale=0.0):
    """max|a-b| / max(max|b|, scale); exact (mpmath) when either side holds mpf objects."""
    a = np.asarray(a).ravel()
    b = np.asarray(b).ravel()
    if a.size == 0:
        return 0.0
    if a.dtype == object or b.dtype == object:
        import mpmath
        num = max(abs(mpmath.mpf(x) - mpmath.mpf(y)) for x, y in zip(a, b))
        den = max([abs(mpmath.mpf(y)) for y in b] + [mpmath.mpf(scale), mpmath.mpf(1e-300)])
        return float(num / den)
    a = a.astype(float)
    b = b.astype(float)
    return float(np.max(np.abs(a - b)) / max(1e-300, float(np.max(np.abs(b))), scale))


def poly_min_instance(pk, coef=(2.0, 1.0, -3.0, 0.0, 1.0)):
    """max y s.t. p(x) - y is a sum of squares (univariate): optimum = min_x p(x).
    One cluster, m = 1, v_k = (1, x_k, x_k^2), lambda = 1, B = 1, c_k = p(x_k), b = 1."""
    N = len(coef)
    deg = (len(coef) - 1) // 2
    xs = np.cos(np.pi * (2 * np.arange(N) + 1) / (2 * N)) * 2.0
    A = [[[np.array([x ** i for i in range(deg + 1)])] for x in xs]]
    H = [[[1.0] for _ in xs]]
    B = np.ones((N, 1))
    c = np.array([np.polyval(list(coef)[::-1], x) for x in xs])
    dcoef = [i * coef[i] for i in range(1, len(coef))]
    r = np.roots(dcoef[::-1])
    r = r[np.abs(r.imag) < 1e-12].real
    pmin = float(min(np.polyval(list(coef)[::-1], r)))
    return [pk.Cluster(A, B, c, H)], np.array([1.0]), pmin


def stage_reference(it, nxt, bi):
    """The oracle's stage outputs of one iteration (``oracle.iteration``'s intermediates ``it``
    and new state ``nxt``) as flat arrays in the C-ABI buffer layout, in stage order.  Names
    match :func:`stage_device`."""
    from clrsdp_amd import instance as inst
    fl = inst.blocks_to_flat
    ay = [it["A_Y"][j][l][r][s] for j in range(bi.J) for l in range(bi.L[j])
          for r in range(bi.m[j]) for s in range(r + 1)]
    out = {"mu": np.array([it["mu"]], dtype=object), "R": fl(it["R"]), "Xinv": fl(it["X_inv"]),
           "S": np.concatenate([s.reshape(-1, order="F") for s in it["dec"].S_raw]),
           "A_Y": np.concatenate(ay), "Q": it["dec"].Q_raw.reshape(-1, order="F"),
           "P": fl(it["P"]), "p": np.asarray(it["p"]), "d": np.asarray(it["d"])}
    for key in ("pred", "corr"):
        if key == "corr":
            out["beta_c"] = np.array([it["beta_c"]], dtype=object)
            out["R2"] = fl(it["R2"])
        dx, dX, dy, dY = it[key]
        out[key + "_dx"], out[key + "_dy"] = np.asarray(dx), np.asarray(dy)
        out[key + "_dX"], out[key + "_dY"] = fl(dX), fl(dY)
    out["alpha_p"] = np.array([it["alpha_p"]], dtype=object)
    out["alpha_d"] = np.array([it["alpha_d"]], dtype=object)
    out["x+"], out["X+"] = np.asarray(nxt[0]), fl(nxt[1])
    out["y+"], out["Y+"] = np.asarray(nxt[2]), fl(nxt[3])
    return out


def stage_device(dev, exact):
    """Run the ten stages of one iteration on a DeviceSolver whose state is set, reading every
    stage's buffers back (the C-ABI layout of :func:`stage_reference`)."""
    from clrsdp_amd import _lib as L
    from clrsdp_amd import instance as inst
    import _clrsdp_pkg
    pk = _clrsdp_pkg.load()
    P = pk.make_params("0.3", "0.1", "0.7", 0)
    buf = lambda k: np.array(dev.buffer(k, exact), dtype=object if exact else float)
    o = {}
    dev.run_stage(L.STAGE_MU_R, P, False)
    o["mu"] = np.array([dev.scalar("mu", exact)], dtype=object)
    o["R"] = buf(L.BUF_R)
    dev.run_stage(L.STAGE_XINV, P, False)
    o["Xinv"] = buf(L.BUF_XINV)
    dev.run_stage(L.STAGE_SCHUR, P, False)
    o["S"], o["A_Y"] = buf(L.BUF_S), buf(L.BUF_AY)
    dev.run_stage(L.STAGE_FACTOR, P, False)
    o["Q"] = buf(L.BUF_Q)
    dev.run_stage(L.STAGE_RESIDUALS, P, False)
    o["P"], o["p"], o["d"] = buf(L.BUF_P), buf(L.BUF_PVEC), buf(L.BUF_DVEC)
    for stage, key in ((L.STAGE_PREDICTOR, "pred"), (L.STAGE_CORRECTOR, "corr")):
        if key == "corr":
            dev.run_stage(L.STAGE_CORRECTOR_R, P, False)
            o["beta_c"] = np.array([dev.scalar("beta_c", exact)], dtype=object)
            o["R2"] = buf(L.BUF_R)
        dev.run_stage(stage, P, False)
        o[key + "_dx"], o[key + "_dy"] = buf(L.BUF_DX), buf(L.BUF_DY)
        o[key + "_dX"], o[key + "_dY"] = buf(L.BUF_DXMAT), buf(L.BUF_DYMAT)
    dev.run_stage(L.STAGE_STEP, P, False)
    o["alpha_p"] = np.array([dev.scalar("alpha_p", exact)], dtype=object)
    o["alpha_d"] = np.array([dev.scalar("alpha_d", exact)], dtype=object)
    dev.run_stage(L.STAGE_UPDATE, P, False)
    xg, Xg, yg, Yg = dev.get_state(exact)
    o["x+"], o["X+"] = np.asarray(xg), inst.blocks_to_flat(Xg)
    o["y+"], o["Y+"] = np.asarray(yg), inst.blocks_to_flat(Yg)
    return o


def residual_scales(cons, b, X):
    """Scales for the residual buffers, which are themselves at round-off level once feasible:
    P against the X scale, p against b, d against c."""
    from clrsdp_amd import instance as inst
    Xscale = float(np.max(np.abs(np.array(inst.blocks_to_flat(X), dtype=float))))
    return {"P": Xscale, "p": float(np.max(np.abs(np.array(b, dtype=float)))),
            "d": float(max(np.max(np.abs(np.array(c.c, dtype=float))) for c in cons))}


# ---- per-piece comparison of the stage buffers (mixed instances) -----------------------------
BLOCK_KEYS = ("R", "Xinv", "P", "R2", "pred_dX", "pred_dY", "corr_dX", "corr_dY", "X+", "Y+")
CLUSTER_KEYS = ("d", "pred_dx", "corr_dx", "x+")


def stage_pieces(bi):
    """{key: [(piece, start, stop)]} for every key of :func:`stage_reference`: the slices of the
    flat C-ABI buffers that belong to one block (``"j<j>l<l>"``: R, Xinv, P, R2, the dX / dY of
    both directions, X+, Y+), one (r,s) slot of one block (``"j<j>l<l>r<r>s<s>"``: A_Y, one entry
    per vector of the block, K = sum of its ranks), one cluster (``"j<j>"``: S with dim_S^2 entries, d, the dx of both directions and x+
    with dim_S), or the whole buffer (``"all"``: Q, p, the dy, y+ and the scalars)."""
    blk, ay, S, xs = [], [], [], []
    ob = oa = oS = 0
    for j in range(bi.J):
        D = bi.dim_S[j]
        S.append((f"j{j}", oS, oS + D * D))
        oS += D * D
        xs.append((f"j{j}", bi.x_indices[j], bi.x_indices[j + 1]))
        for l in range(bi.L[j]):
            n, K = bi.Y_blocksizes[j][l], bi.rank_sums[j][l][-1]
            blk.append((f"j{j}l{l}", ob, ob + n * n))
            ob += n * n
            for r in range(bi.m[j]):
                for s in range(r + 1):
                    ay.append((f"j{j}l{l}r{r}s{s}", oa, oa + K))
                    oa += K
    out = {k: blk for k in BLOCK_KEYS}
    out.update({k: xs for k in CLUSTER_KEYS})
    out["S"], out["A_Y"] = S, ay
    ny = bi.n_y
    for k, n in (("Q", ny * ny), ("p", ny), ("pred_dy", ny), ("corr_dy", ny), ("y+", ny), ("mu", 1),
                 ("beta_c", 1), ("alpha_p", 1), ("alpha_d", 1)):
        out[k] = [("all", 0, n)]
    return out


def piecewise_err(got, ref, bi, scales=None):
    """{(key, piece): rel_err} of the stage buffers ``got`` against ``ref`` (the dictionaries of
    :func:`stage_device` and :func:`stage_reference`), every piece of :func:`stage_pieces`
    relative to its own largest reference entry, so that an error confined to a small cluster is
    not hidden under a large cluster's scale.  ``scales`` (:func:`residual_scales`) keeps the
    floor of the residual buffers P, p, d, which are at round-off level once feasible."""
    scales = scales or {}
    out = {}
    for key, pieces in stage_pieces(bi).items():
        if key not in ref:
            continue
        g, r = np.asarray(got[key]).ravel(), np.asarray(ref[key]).ravel()
        assert len(g) == len(r) == pieces[-1][2], (key, len(g), len(r), pieces[-1][2])
        for piece, a, c in pieces:
            out[(key, piece)] = rel_err(g[a:c], r[a:c], scales.get(key, 0.0))
    return out


def summarize_pieces(ref, bi, digits, count=384):
    """Fixture records of the stage buffers per piece: {key: {piece: summarize(slice)}}."""
    return {key: {piece: summarize(np.asarray(ref[key], dtype=object).ravel()[a:c], digits, count)
                  for piece, a, c in pieces}
            for key, pieces in stage_pieces(bi).items() if key in ref}


def compare_pieces(got, recs, bi, scales=None):
    """{(key, piece): compare_summary} of stage buffers against :func:`summarize_pieces` records."""
    scales = scales or {}
    out = {}
    for key, pieces in stage_pieces(bi).items():
        if key not in recs:
            continue
        g = np.asarray(got[key], dtype=object).ravel()
        assert len(g) == pieces[-1][2], (key, len(g), pieces[-1][2])
        for piece, a, c in pieces:
            out[(key, piece)] = compare_summary(g[a:c], recs[key][piece], scales.get(key, 0.0))
    return out


def worst(errs, tol):
    """(error / tolerance, key) of the worst piece of a {key: error} dictionary; ``tol`` a number
    or a dictionary over the same keys."""
    t = (lambda k: tol[k]) if isinstance(tol, dict) else (lambda k: tol)
    return max(((v / t(k), k) for k, v in errs.items()), key=lambda q: q[0] if q[0] == q[0] else np.inf)


# ---- mixed instances: pk.synth_mixed(specs, n_y, seed=7) --------------------------------------
def _sp(m, deltas, N, ranks=None):
    return dict(m=m, deltas=list(deltas), N=N, ranks=ranks)


_R3 = [[(1, 2, 1, 3, 1, 2)[k % 6] for k in range(47)]]
# (no sample has rank 0 in both blocks)
_RZ = [[(0, 1, 2, 1)[k % 4] for k in range(79)],
       [((1, 2)[k % 8 == 0] if k % 4 == 0 else (1, 0, 2)[k % 3]) for k in range(79)]]
_MS = [_sp(1, [20], 39), _sp(1, [100], 199), _sp(1, [70], 139), _sp(1, [12], 23)]
_MT = [_sp(1, [40], 79), _sp(1, [33], 65, [[2] * 65]), _sp(1, [24], 47, _R3), _sp(1, [40, 24], 79, _RZ)]
MIXED = {
    "M-S": (_MS, 24),
    "M-S+": (_MS + [_sp(1, [140], 279)], 24),
    "M-T": (_MT, 24),
    "M-Q": (_MT, 140),
    "M-m": ([_sp(1, [70], 139), _sp(2, [30, 20], 59), _sp(1, [100], 199)], 24),
    "M-bS": ([_sp(3, [30], 59), _sp(1, [20], 39)], 16),
    "M-Bs": ([_sp(1, [140], 150), _sp(1, [20], 39)], 16),
    # the multi-word fixtures (tests/golden/make_stage_fixtures.py) and their split-form variants
    "mixdd": ([_sp(1, [12], 23), _sp(1, [70], 139), _sp(1, [40, 24], 79, _RZ)], 70),
    "mixdds": ([_sp(1, [12], 23), _sp(1, [40, 24], 79, _RZ)], 70),
    "mixqd": ([_sp(1, [8], 15), _sp(1, [36], 71), _sp(2, [10, 6], 19)], 40),
    "mixqds": ([_sp(1, [8], 15), _sp(2, [10, 6], 19)], 40),
}
_MIXED_STATES = {}


def mixed_instance(pk, name):
    specs, n_y = MIXED[name]
    return pk.synth_mixed(specs, n_y, seed=7)


def mixed_oracle_case(pk, oracle, name, iters_before=2):
    """(cons, b, bi, state, nxt, it) of a mixed instance: the numpy oracle's state after
    ``iters_before`` iterations from initial_point(.., 10, 10) and its next iteration, computed
    once per instance and left unchanged."""
    if name not in _MIXED_STATES:
        cons, b = mixed_instance(pk, name)
        bi = oracle.get_block_info(cons)
        ar = oracle.Fp64()
        prm = {k: oracle._param(ar, v) for k, v in oracle.DEFAULTS.items()}
        state = oracle.initial_point(ar, bi, 10.0, 10.0)
        for _ in range(iters_before):
            state, _ = oracle.iteration(ar, cons, bi, b, None, ar.num(0), state, False, prm)
        nxt, it = oracle.iteration(ar, cons, bi, b, None, ar.num(0), state, False, prm)
        _MIXED_STATES[name] = (cons, b, bi, state, nxt, it)
    return _MIXED_STATES[name]


def _sample_sums(M, starts, counts):
    """Sums of the rows and columns of the K x K matrix M over the rank groups of the samples
    (N x N): group k holds rows starts[k] .. starts[k] + counts[k] - 1 (none when the rank is 0)."""
    nz = counts > 0
    out = np.zeros((len(counts), len(counts)), dtype=M.dtype)
    if nz.any():
        R = np.add.reduceat(M, starts[nz], axis=0)
        out[np.ix_(nz, nz)] = np.add.reduceat(R, starts[nz], axis=1)
    return out


def _ld_gemm_nt(A, Bt, threads=8):
    """A @ Bt.T for C-contiguous longdouble A (M x k) and Bt (N x k).  numpy has no BLAS for
    longdouble; its einsum loop over two contiguous rows is the fastest form it has, and it
    releases the GIL, so row slabs of A go to a few threads (K = 4098, k = 65: 0.4 s against the
    4.5 s of V.T @ TX).  The sums of each entry are the same whatever the slabs."""
    from concurrent.futures import ThreadPoolExecutor
    A, Bt = np.ascontiguousarray(A), np.ascontiguousarray(Bt)
    out = np.empty((A.shape[0], Bt.shape[0]), dtype=A.dtype)
    if A.shape[0] * Bt.shape[0] < 1 << 16:
        out[...] = np.einsum("ik,jk->ij", A, Bt)
        return out
    edges = np.linspace(0, A.shape[0], 4 * threads + 1).astype(int)

    def slab(q):
        out[edges[q]:edges[q + 1]] = np.einsum("ik,jk->ij", A[edges[q]:edges[q + 1]], Bt)
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(slab, range(4 * threads)))
    return out


def schur_dense(cons, bi, X_inv, Y, dtype=np.longdouble):
    """Dense restatement of the SCHUR stage (the 4-term formula, MPMP.jl:1373-1398, as
    oracle/mpmp_oracle.py:compute_S_integrated assembles it): V, X^-1 and Y taken as float64, every
    product and sum accumulated in np.longdouble, all of it as GEMMs, Hadamard products and group
    sums -- usable at K of several thousand, where the oracle's per-entry code is not.
    Returns (S, A_Y) as flat longdouble arrays in the layout of BUF_S and BUF_AY.  ``dtype``
    np.float64 gives the plain float64 restatement of the same formula (tests/schur_cases.py)."""
    ld = dtype
    S_out, AY_out = [], []
    for j in range(bi.J):
        m, N, D = bi.m[j], bi.n_samples[j], bi.dim_S[j]
        Sj = np.zeros((D, D), dtype=ld)
        for l in range(bi.L[j]):
            cl = cons[j]
            V = np.stack([np.asarray(v, dtype=np.float64) for vk in cl.A[l] for v in vk], axis=1).astype(ld)
            lam = np.array([float(x) for hk in cl.H[l] for x in hk], dtype=np.float64).astype(ld)
            counts = np.array([len(vk) for vk in cl.A[l]], dtype=np.int64)
            starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
            delta, K = V.shape
            Xi = np.asarray(X_inv[j][l], dtype=np.float64).astype(ld)
            Yb = np.asarray(Y[j][l], dtype=np.float64).astype(ld)
            blk = lambda M, r, s: M[r * delta:(r + 1) * delta, s * delta:(s + 1) * delta]
            Vt = np.ascontiguousarray(V.T)
            BX = [[_ld_gemm_nt(Vt, (blk(Xi, r, s) @ V).T) for s in range(m)] for r in range(m)]
            BY = [[_ld_gemm_nt(Vt, (blk(Yb, r, s) @ V).T) for s in range(m)] for r in range(m)]
            AY_out += [np.diagonal(BY[r][s]).copy() for r in range(m) for s in range(r + 1)]
            LL = np.outer(lam, lam) / 4
            for r1 in range(m):
                for s1 in range(r1 + 1):
                    for r2 in range(m):
                        for s2 in range(r2 + 1):
                            T = (BX[s1][r2] * BY[s2][r1].T + BX[r1][r2] * BY[s2][s1].T
                                 + BX[s1][s2] * BY[r2][r1].T + BX[r1][s2] * BY[r2][s1].T)
                            h0 = (s1 + r1 * (r1 + 1) // 2) * N
                            v0 = (s2 + r2 * (r2 + 1) // 2) * N
                            Sj[v0:v0 + N, h0:h0 + N] += _sample_sums(LL * T, starts, counts).T
        Sup = np.triu(Sj)   # Symmetric(S_j) from its upper triangle (MPMP.jl:1409)
        S_out.append((Sup + np.triu(Sj, 1).T).reshape(-1, order="F"))
    return np.concatenate(S_out), np.concatenate(AY_out)


# ---- graded data: componentwise parity of the Schur products --------------------------------
def graded_instance(pk, delta, rank, N, g, seed):
    """One m = 1 cluster on the grading a monomial-type basis gives an interior-point iterate:
    synth's V, lambda and B with component i of every v multiplied by 2^(-g i) (exact), and a
    state X = D Mx D, Y = D^-1 My D^-1 with D = diag(2^(-g i)) and Mx, My seeded SPD (rand_spd,
    symmetric float64; the scalings are exact too).  Not feasible -- for the MU_R, XINV and SCHUR
    stages only.  Returns (constraints, b, (x, X, y, Y))."""
    cons, b = pk.synth(seed=seed, J=1, L=1, delta=delta, rank=rank, n_y=2, N=N)
    d = np.ldexp(1.0, -g * np.arange(delta))
    cl = cons[0]
    cl.A = [[[np.asarray(v, dtype=float) * d for v in vk] for vk in cl.A[0]]]
    rng = np.random.default_rng(seed)
    sym = lambda M: (M + M.T) / 2
    Mx, My = sym(rand_spd(delta, rng)), sym(rand_spd(delta, rng))
    X = d[:, None] * Mx * d[None, :]
    Y = My / d[:, None] / d[None, :]
    return cons, b, (np.zeros(N), [[X]], np.zeros(2), [[Y]])


def _exact_ints(a):
    """(object array of Python ints I, exponent e) with a = I 2^e exactly, for an array of
    float64 or mpmath.mpf values."""
    import mpmath
    a = np.asarray(a)
    parts = []
    for v in a.ravel():
        sign, man, exp, _ = (v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v)))._mpf_
        parts.append((-int(man) if sign else int(man), int(exp)))
    e = min([ex for mn, ex in parts if mn] + [0])
    out = np.empty(a.size, dtype=object)
    for i, (mn, ex) in enumerate(parts):
        out[i] = mn << (ex - e) if mn else 0
    return out.reshape(a.shape), e


def schur_exact(cl, X_inv, Y, prec=256):
    """S and A_Y of one m = 1, L = 1 cluster from the given X^-1 (float64 or mpf entries, e.g. a
    device's own), Y, V and lambda (float64): the 4-term formula (MPMP.jl:1373-1398) at m = 1,
    S[k2, k1] = sum lambda_1 lambda_2 BX[rho_1, rho_2] BY[rho_2, rho_1] over rho_i in sample k_i,
    upper triangle mirrored, A_Y = diag(BY), with BX = V^T X^-1 V and BY = V^T Y V.  Every
    operand is a dyadic rational, so all of it is done in exact integer arithmetic and rounded
    once to ``prec`` bits of mpmath.mpf.  Also returns the componentwise bounds of both (float64):
    the same formulas with every factor replaced by its absolute value."""
    import mpmath
    V = np.stack([np.asarray(v, dtype=float) for vk in cl.A[0] for v in vk], axis=1)
    lam = np.array([float(x) for hk in cl.H[0] for x in hk])
    counts = np.array([len(vk) for vk in cl.A[0]], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    Vi, ev = _exact_ints(V)
    Xi, ex = _exact_ints(X_inv)
    Yi, ey = _exact_ints(Y)
    li, el = _exact_ints(lam)
    BX = Vi.T @ (Xi @ Vi)
    BY = Vi.T @ (Yi @ Vi)
    Sg = _sample_sums(np.outer(li, li) * (BX * BY.T), starts, counts).T
    N = len(counts)
    iu = np.triu_indices(N, 1)
    Sg[(iu[1], iu[0])] = Sg[iu]
    eS, eA = 2 * el + 4 * ev + ex + ey, 2 * ev + ey
    with mpmath.workprec(prec):
        S = np.array([mpmath.ldexp(mpmath.mpf(int(v)), eS) for v in Sg.reshape(-1, order="F")], dtype=object)
        AY = np.array([mpmath.ldexp(mpmath.mpf(int(v)), eA) for v in np.diagonal(BY)], dtype=object)
    aV = np.abs(V)
    absf = lambda M: np.abs(np.array([[float(v) for v in r] for r in np.asarray(M)]))
    bX, bY = aV.T @ absf(X_inv) @ aV, aV.T @ absf(Y) @ aV
    bS = _sample_sums(np.outer(np.abs(lam), np.abs(lam)) * (bX * bY.T), starts, counts).T
    bS[(iu[1], iu[0])] = bS[iu]
    return S, AY, bS.reshape(-1, order="F"), np.diagonal(bY).copy()


def cw_err(got, ref, bound):
    """Componentwise error: the maximum over entries of |got - ref| / bound, in mpmath at 320
    bits (whatever the global precision is)."""
    import mpmath
    g, r = np.asarray(got, dtype=object).ravel(), np.asarray(ref, dtype=object).ravel()
    bd = np.asarray(bound, dtype=float).ravel()
    assert len(g) == len(r) == len(bd)
    with mpmath.workprec(320):
        return float(max([abs(mpmath.mpf(x) - mpmath.mpf(y)) / mpmath.mpf(float(s))
                          for x, y, s in zip(g, r, bd)] + [mpmath.mpf(0)]))


# ---- eigenvalue references without an eigen-solve ---------------------------------------------
def known_spectrum(n, lam, rng, reflectors=3):
    """Symmetric n x n object array of 320-bit mpmath numbers with the eigenvalues ``lam``:
    H_r .. H_1 diag(lam) H_1 .. H_r with H = I - 2 u u^T / u^T u and u random (float64 entries).
    Each reflector is applied as the symmetric rank-2 update A - u w^T - w u^T (p = beta A u,
    K = beta u^T p / 2, w = p - K u), O(n^2) per reflector.  The lower triangle is copied over the
    upper one (the roundings leave ~1e-97 of asymmetry).  lambda_min is min(lam) by construction,
    to the 320-bit rounding of O(n) orthogonal updates (~n 2^-320 ||A||)."""
    import mpmath
    assert len(lam) == n
    with mpmath.workprec(320):
        A = np.empty((n, n), dtype=object)
        A[...] = mpmath.mpf(0)
        for i in range(n):
            A[i, i] = mpmath.mpf(lam[i])
        for _ in range(reflectors if n > 1 else 0):
            u = np.array([mpmath.mpf(float(x)) for x in rng.standard_normal(n)], dtype=object)
            beta = 2 / mpmath.fsum(x * x for x in u)
            p = A.dot(u) * beta
            K = beta * mpmath.fsum(x * y for x, y in zip(u, p)) / 2
            w = p - K * u
            A = A - np.outer(u, w) - np.outer(w, u)
        il = np.tril_indices(n, -1)
        A[(il[1], il[0])] = A[il]
    return A


def neg_pivots(M):
    """Number of negative pivots of the L D L^T factorisation without pivoting of the symmetric
    matrix M (object array of mpmath numbers or floats; only the lower triangle is read), at 320
    bits.  By Sylvester's law of inertia that is the number of negative eigenvalues of M, and for
    M = dM - sigma B with B positive definite the number of generalised eigenvalues of (dM, B)
    below sigma.  A zero pivot is refused (the count would be undefined)."""
    import mpmath
    n = len(M)
    with mpmath.workprec(320):
        A = np.empty((n, n), dtype=object)
        A[...] = mpmath.mpf(0)
        for i in range(n):
            for j in range(i + 1):
                A[i, j] = mpmath.mpf(M[i][j])
        neg = 0
        for k in range(n):
            d = A[k, k]
            assert d != 0, f"neg_pivots: zero pivot {k}"
            neg += d < 0
            col = A[k + 1:, k]
            # (the whole outer product in one numpy call is faster than row slices of its
            # lower triangle: 1.6 s against 2.3 s at n = 100)
            A[k + 1:, k + 1:] -= np.tril(np.outer(col / d, col))
    return int(neg)


# ---- sampled fixtures of large stage outputs (tests/golden/make_stage_fixtures.py) ----------
SKETCH_MULT = (0x9E3779B1, 0x85EBCA77)


def sketch_weights(n, which):
    """Deterministic +-1 weights for the linear sketch number ``which`` of an n-vector."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (i + np.uint64(1)) * np.uint64(SKETCH_MULT[which]) & np.uint64(0xFFFFFFFF)
    return 1 - 2 * ((h >> np.uint64(13)) & np.uint64(1)).astype(np.int64)


def sample_indices(n, count=384, seed=2024):
    """Sorted sample of indices: the first and last 32 entries and ``count`` spread by a
    fixed multiplicative hash (no RNG, identical on every host)."""
    if n <= count + 64:
        return list(range(n))
    s = set(range(32)) | set(range(n - 32, n))
    k = 0
    while len(s) < count + 64:
        s.add(int((k * 2654435761 + seed * 40503) % n))
        k += 1
    return sorted(s)


def summarize(arr, digits, count=384):
    """Fixture record of a flat buffer: sampled entries (``count`` + 64 of them), two +-1
    sketches, the l1 norm and the max |entry| (decimal strings at ``digits`` significant digits)."""
    import mpmath
    a = [mpmath.mpf(v) for v in np.asarray(arr, dtype=object).ravel()]
    n = len(a)
    idx = sample_indices(n, count)
    st = lambda v: mpmath.nstr(v, digits, strip_zeros=False, min_fixed=1, max_fixed=0)
    rec = {"n": n, "idx": idx, "val": [st(a[i]) for i in idx],
           "l1": st(mpmath.fsum(abs(v) for v in a)), "amax": st(max([abs(v) for v in a] + [mpmath.mpf(0)]))}
    rec["sketch"] = [st(mpmath.fsum(int(w) * v for w, v in zip(sketch_weights(n, q), a))) for q in range(2)]
    return rec


def compare_summary(arr, rec, scale=0.0):
    """Scale-aware relative error of a device buffer against a fixture record: max over the
    sampled entries (relative to max(amax, scale)) and the sketches (relative to l1)."""
    import mpmath
    a = np.asarray(arr, dtype=object).ravel()
    assert len(a) == rec["n"], (len(a), rec["n"])
    # the fixture strings are parsed and the differences taken at 320 bits whatever the global
    # mpmath.mp.prec is (a test run that starts with this comparison has it at 53)
    with mpmath.workprec(320):
        den = max(mpmath.mpf(rec["amax"]), mpmath.mpf(scale), mpmath.mpf(1e-300))
        err = max([abs(mpmath.mpf(a[i]) - mpmath.mpf(v)) / den
                   for i, v in zip(rec["idx"], rec["val"])] + [mpmath.mpf(0)])
        l1 = max(mpmath.mpf(rec["l1"]), mpmath.mpf(scale) * len(a), mpmath.mpf(1e-300))
        for q, sv in enumerate(rec["sketch"]):
            s = mpmath.fsum(int(w) * mpmath.mpf(v) for w, v in zip(sketch_weights(len(a), q), a))
            err = max(err, abs(s - mpmath.mpf(sv)) / l1)
    return float(err)


CONFIGS_SMALL = [
    dict(J=2, delta=4, rank=1, n_y=4),                    # C1
    dict(J=2, delta=3, rank=1, n_y=3, m=2, L=2),          # polynomial-matrix clusters, 2 blocks
    dict(J=3, delta=4, rank=2, n_y=5),                    # rank 2
    dict(J=3, delta=5, rank=1, n_y=4, m=3, L=2),          # m = 3
    dict(J=1, delta=6, rank=1, n_y=1),                    # single cluster, n_y = 1
]
