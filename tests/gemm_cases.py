"""Inputs, exact references and a-priori bounds of the product tests (test_gemm_host.py on the
CPU, test_gpu_gemm.py and test_gpu_gemm_chain.py on the GPU).

Operands are raw limbs of shape (words, rows, columns); the number under test is the limb sum, a
dyadic rational, so every reference here is exact: the limbs become Python integers times a power
of two, the products are numpy object-array products of those integers, and one rounding to 320
bits of mpmath.mpf ends it (relative 2^-320 of the entry itself).

Operand classes (``operands(kind, ...)`` returns op(A) and op(B); a test stores the transpose
where the launch reads one):
  random  every limb random at its natural magnitude (limb q ~ 2^-53q), normalised by error-free
          sums; no entry is zero, so the last k-term, the last row and the last column count
  graded  random with row i of op(A) scaled by 2^-(i mod 40) and column j of op(B) likewise
          (potrf_cases.dscale, exact): entries of C span 2^-78, the bound must be componentwise
  cancel  leading magnitudes in [1/2, 1), column 2m+1 of op(A) = -(1 + r 2^-31) column 2m, row
          2m+1 of op(B) = row 2m, an unpaired last term scaled by 2^-33:
          |sum a b| <= 2^-30 sum |a||b| for K >= 2, so C consists of what the low bits leave
  exact   integers of magnitude 1 .. 8 times powers of two per row / column (at words > 1 plus a
          second integer at 2^-70 in op(A)): every partial sum in any order is representable,
          the result must be the reference in every limb

Bound, u = EPS[words]:
  |C - C^|_ij <= (K + extra) u (|alpha| (|op A||op B|)_ij + |beta Cin_ij| + |dmult s| [i = j])
with extra = 4 (6 for the scaled-A form, whose |op A| carries |sa sl|).
"""
import mpmath
import numpy as np

from potrf_cases import EPS, dscale

PREC = 320
KINDS = ("random", "graded", "cancel", "exact")


def _uniform(seed, stream, shape):
    from clrsdp_amd import instance as inst
    return inst.uniform(seed, stream, int(np.prod(shape))).reshape(shape)


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def renorm(terms, words):
    """(words, ...) non-overlapping limbs from float terms of decreasing magnitude: bottom-up
    error-free sweeps, the leading `words` results kept (the value under test is their sum)"""
    t = [np.array(x, dtype=np.float64) for x in terms]
    while len(t) < words:
        t.append(np.zeros_like(t[0]))
    for _ in range(len(t)):
        for q in range(len(t) - 1, 0, -1):
            t[q - 1], t[q] = two_sum(t[q - 1], t[q])
    out = np.stack(t[:words])
    for q in range(words - 1):
        assert np.all(out[q] + out[q + 1] == out[q]), "limbs overlap"
    return out


def _terms(shape, words, seed, stream, half=False):
    out = []
    for t in range(words):
        u = _uniform(seed, stream + t, shape)
        if t == 0:
            # no zero entry; `half`: magnitudes in [1/2, 1)
            u = np.where(u >= 0, 1.0, -1.0) * (0.5 + 0.5 * np.abs(u)) if half else np.where(u == 0.0, 0.5, u)
        out.append(u * 2.0 ** (-53 * t))
    return out


def _small_ints(shape, seed, stream):
    u = _uniform(seed, stream, shape)
    return np.where(u >= 0, 1.0, -1.0) * (1.0 + np.floor(np.abs(u) * 8.0).clip(0, 7))


def operands(kind, M, N, K, words, seed):
    """limbs of op(A) (words, M, K) and op(B) (words, K, N)"""
    if kind == "exact":
        A = np.zeros((words, M, K))
        B = np.zeros((words, K, N))
        ra = 2.0 ** ((np.arange(M) % 7) - 3)[:, None]
        A[0] = _small_ints((M, K), seed, 40) * ra
        B[0] = _small_ints((K, N), seed, 41) * 2.0 ** ((np.arange(N) % 5) - 2)[None, :]
        if words > 1:
            A[1] = _small_ints((M, K), seed, 42) * ra * 2.0 ** -70
        return A, B
    ta = _terms((M, K), words, seed, 10, half=kind == "cancel")
    tb = _terms((K, N), words, seed, 20, half=kind == "cancel")
    if kind == "cancel" and K >= 2:
        odd = np.arange(1, K, 2)
        r = _uniform(seed, 30, (M, len(odd)))
        for t in ta:
            t[:, odd] = -t[:, odd - 1]
        ta.append(np.zeros((M, K)))
        ta[-1][:, odd] = -ta[0][:, odd - 1] * r * 2.0 ** -31
        ta.sort(key=lambda x: -np.max(np.abs(x)))
        for t in tb:
            t[odd, :] = t[odd - 1, :]
        if K % 2:
            for t in ta:
                t[:, K - 1] *= 2.0 ** -33
    A, B = renorm(ta, words), renorm(tb, words)
    if kind == "graded":
        A = A * dscale(M)[None, :, None]
        B = B * dscale(N)[None, None, :]
    return A, B


def matrix(kind, M, N, words, seed, stream=50):
    """limbs (words, M, N) of a C_in of the class's scale"""
    if kind == "exact":
        C = np.zeros((words, M, N))
        C[0] = _small_ints((M, N), seed, stream) * (2.0 ** ((np.arange(M) % 7) - 3)[:, None]
                                                      * 2.0 ** ((np.arange(N) % 5) - 2)[None, :])
        return C
    C = renorm(_terms((M, N), words, seed, stream), words)
    if kind == "graded":
        C = C * (dscale(M)[:, None] * dscale(N)[None, :])[None]
    return C


# ---- exact arithmetic ---------------------------------------------------------------------------
def ints(limbs):
    """(I, e): the limb sums of (words, rows, columns) limbs -- or, of a 1-D or 2-D float array,
    its entries -- as an object array of Python integers times 2^e (vectorised frexp;
    test_gemm_host.py checks it against helpers._exact_ints)"""
    limbs = np.asarray(limbs, dtype=np.float64)
    assert np.all(np.isfinite(limbs)), "non-finite operand"
    m, ex = np.frexp(limbs)
    mi = np.ldexp(m, 53).astype(np.int64)          # |m| < 1: exact 53-bit integers
    ex = ex.astype(np.int64) - 53
    nz = mi != 0
    e = int(ex[nz].min()) if nz.any() else 0
    sh = np.where(nz, ex - e, 0)
    out = mi.astype(object) << sh.astype(object)
    return out.sum(axis=0) if out.ndim > 2 else out, e


def to_mpf(I, e):
    """object array of mpf: I 2^e rounded once to PREC bits"""
    with mpmath.workprec(PREC):
        f = np.frompyfunc(lambda v: mpmath.ldexp(mpmath.mpf(int(v)), e), 1, 1)
        return f(np.asarray(I, dtype=object))


def limb_sum(limbs):
    """the exact sums of (words, ...) limbs as mpf (PREC bits hold four normalised limbs)"""
    return to_mpf(*ints(limbs))


def split(vals, words):
    """object array of mpf -> (words, ...) limbs, limb q the nearest double of what the limbs
    before it leave over (the canonical limbs of a representable number)"""
    vals = np.asarray(vals, dtype=object)
    out = np.zeros((words,) + vals.shape)
    for idx in np.ndindex(*vals.shape):
        r = vals[idx]
        for q in range(words):
            h = float(r)
            out[(q,) + idx] = h
            r = mpmath.fsub(r, h, exact=True)
    return out


def product(A, B, scale=None):
    """exact op(A) op(B) as (I, e); with `scale`, a float vector or a tuple of them (sa, sl),
    op(A) diag(scale) op(B) with the exact product of the vectors"""
    Ai, ea = ints(A)
    Bi, eb = ints(B)
    for v in (() if scale is None else scale if isinstance(scale, tuple) else (scale,)):
        si, es = ints(np.asarray(v, dtype=np.float64))
        Ai, ea = Ai * si[None, :], ea + es
    return Ai @ Bi, ea + eb


def _axpy(X, ex, a, Y, ey):
    """(a X 2^ex + Y 2^ey) as (I, e) for a float a (Y None: a X alone)"""
    ai, ea = ints(np.array([float(a)]))
    X, ex = X * int(ai[0]), ex + ea
    if Y is None:
        return X, ex
    e = min(ex, ey)
    return (X << (ex - e)) + (Y << (ey - e)), e


def reference_ints(P, alpha=1.0, beta=0.0, Cin=None, diag=0.0):
    """alpha P + beta Cin + diag I exactly, as (I, e); P = (I, e) of product(), Cin limbs, alpha,
    beta and diag floats (diag = dmult * s, formed by the caller where the kernel forms it)"""
    R, e = _axpy(P[0], P[1], alpha, None, 0)
    if beta != 0.0:
        Ci, ec = ints(Cin)
        R, e = _axpy(Ci, ec, beta, R, e)
    if diag != 0.0:
        D = np.zeros(R.shape, dtype=object)
        D[np.diag_indices(min(R.shape))] = 1
        R, e = _axpy(D, 0, diag, R, e)
    return R, e


def reference(P, alpha=1.0, beta=0.0, Cin=None, diag=0.0):
    """reference_ints rounded once to mpf at PREC bits"""
    return to_mpf(*reference_ints(P, alpha, beta, Cin, diag))


def abs1(limbs):
    """|limb sum| to fp64 (the leading limb: relative 2^-53, far inside the bound's constant)"""
    return np.abs(np.asarray(limbs, dtype=np.float64)[0])


def bound(A, B, words, alpha=1.0, beta=0.0, Cin=None, diag=0.0, extra=4, scale=None):
    """the componentwise a-priori bound of the module docstring (float array M x N)"""
    aA = abs1(A)
    for v in (() if scale is None else scale if isinstance(scale, tuple) else (scale,)):
        aA = aA * np.abs(np.asarray(v))[None, :]
    K = aA.shape[1]
    b = abs(alpha) * (aA @ abs1(B))
    if beta != 0.0:
        b = b + np.abs(beta) * abs1(Cin)
    if diag != 0.0:
        b = b + np.abs(diag) * np.eye(*b.shape)
    return (K + extra) * EPS[words] * b


def ratio(got_limbs, ref, bnd, certify=16, mask=None):
    """max |got - ref| / bound over the entries, in mpmath at 320 bits (helpers.cw_err); got as
    limbs (words, M, N), ref an object array of mpf or the exact (I, e) of reference_ints.  With
    (I, e) the differences are first formed exactly in integers for every entry and divided by the
    bound in float64 (relative 2^-52: a screen), and cw_err then decides the `certify` largest --
    so a batch of 10^5 entries costs 16 mpmath comparisons, not 10^5.  A NaN is a failure of its
    own.  ``mask`` (with (I, e) only): the entries that count; the others may hold anything."""
    from helpers import cw_err
    got_limbs = np.asarray(got_limbs, dtype=np.float64)
    if mask is not None:
        got_limbs = np.where(mask[None], got_limbs, 0.0)
    assert not np.isnan(got_limbs).any(), "NaN in the result"
    bnd = np.asarray(bnd, dtype=np.float64)
    assert np.all(bnd > 0.0)
    if not isinstance(ref, tuple):
        assert mask is None
        return cw_err(limb_sum(got_limbs), ref, bnd)
    G, eg = ints(got_limbs)
    R, er = ref
    e = min(eg, er)
    D = abs((G << (eg - e)) - (R << (er - e)))
    screen = np.ldexp(D.astype(np.float64), e) / bnd
    if mask is not None:
        screen = np.where(mask, screen, 0.0)
    top = np.argsort(screen, axis=None)[-certify:]
    idx = np.unravel_index(top, screen.shape)
    if screen[idx].max() == 0.0:
        return 0.0
    sure = cw_err(to_mpf(G[idx], eg), to_mpf(R[idx], er), bnd[idx])
    assert abs(sure - screen.max()) <= 1e-9 * sure, (sure, screen.max())
    return sure


def stored(op, trans):
    """the matrix a launch with the given transpose flag reads op from"""
    return np.ascontiguousarray(op.transpose(0, 2, 1)) if trans else op


# ---- chain_f64 references -----------------------------------------------------------------------
def chain_reference(A1, B1, C1, A2, a1, b1, P=None):
    """exact O = A2 (a1 A1 B1 + b1 C1) as (I, e) (fp64 operands as 2-D float arrays; a1 in
    {-1, 1}, b1 in {-1, 0, 1}; P = product(A1, B1) when the caller has it), the bound -- the
    product bound applied twice,
      |A2| (n + 4) u (|A1||B1| + |b1 C1|)  +  (n + 2) u |A2| (|A1||B1| + |b1 C1|)
    -- and |A2| (|A1||B1| + |b1 C1|), which bounds |O| itself"""
    assert a1 in (-1.0, 1.0) and b1 in (-1.0, 0.0, 1.0)
    n = A1.shape[0]
    P = product(A1[None], B1[None]) if P is None else P
    use_c = b1 != 0.0 and C1 is not None
    T, et = _axpy(P[0], P[1], a1, None, 0)
    if use_c:
        Ci, ec = ints(C1[None])
        T, et = _axpy(Ci, ec, b1, T, et)
    A2i, e2 = ints(A2[None])
    That = np.abs(A1) @ np.abs(B1) + (np.abs(C1) if use_c else 0.0)
    absO = np.abs(A2) @ That
    u = EPS[1]
    return (A2i @ T, e2 + et), ((n + 4) + (n + 2)) * u * absO, absO


def known_lower(n, seed):
    """an L^-1-like lower triangular factor with exact zeros above the diagonal: random below,
    graded like potrf_cases.known_factor's inverse (row i scaled by 2^(i mod 40))"""
    L = np.tril(_uniform(seed, 60, (n, n)))
    L[np.diag_indices(n)] = 1.0 + np.abs(np.diag(L))
    return L * (1.0 / dscale(n))[:, None]


def sym_matrix(n, seed, graded=True):
    M = _uniform(seed, 61, (n, n))
    M = np.tril(M) + np.tril(M, -1).T
    d = dscale(n)
    return M * (d[:, None] * d[None, :]) if graded else M


def congruence_reference(L, M):
    """exact L M L^T as mpf and its bound (the product bound twice, as chain_reference)"""
    O, bnd, _ = chain_reference(M, np.ascontiguousarray(L.T), None, L, 1.0, 0.0)
    return to_mpf(*O), bnd


def dot_reference(DA, DdA, DB, O, bO, absO):
    """exact <DA + DdA, DB + O> for the exact O = (I, e) of chain_reference, as (I, e) of one
    number, and the bound of the sum of one problem's partials: every partial is a sum of at most
    32 n products of two rounded sums, in some order,
      (32 n + 4) u sum (|DA| + |DdA|) (|DB| + |O|)  +  sum (|DA| + |DdA|) bound(O)"""
    n = DA.shape[0]
    Xa, ea = ints(DA[None])
    Xd, ed = ints(DdA[None])
    X, ex = _axpy(Xa, ea, 1.0, Xd, ed)
    Yb, eb = ints(DB[None])
    Y, ey = _axpy(Yb, eb, 1.0, O[0], O[1])
    aX = np.abs(DA) + np.abs(DdA)
    bnd = (32 * n + 4) * EPS[1] * float(np.sum(aX * (np.abs(DB) + absO))) + float(np.sum(aX * bO))
    return (np.array([[(X * Y).sum()]], dtype=object), ex + ey), np.array([[bnd]])


def trace_reference(Z, V, lam, din, c_agg, c_in):
    """exact rout[t] = c_agg lam[t] ((Z V)[:, t] . V[:, t]) + c_in din[t] as (I, e) (1 x NC) and
    the bound: the product bound for U = Z V, once more for the column dot, and the C_in term,
      |c_agg lam_t| 2 (n + 4) u ((|Z||V|)^T |V|)_tt  +  (n + 4) u |c_in din_t|"""
    n = Z.shape[0]
    U, eu = product(Z[None], V[None])
    Vi, ev = ints(V[None])
    li, el = ints(np.asarray(lam, dtype=np.float64))
    R, e = _axpy((U * Vi).sum(axis=0) * li, eu + ev + el, c_agg, None, 0)
    bnd = np.abs(c_agg * lam) * 2 * (n + 4) * EPS[1] * np.sum((np.abs(Z) @ np.abs(V)) * np.abs(V), axis=0)
    if din is not None:
        di, ed = ints(np.asarray(din, dtype=np.float64))
        R, e = _axpy(di, ed, c_in, R, e)
        bnd = bnd + (n + 4) * EPS[1] * np.abs(c_in * din)
    return (R[None, :], e), bnd[None, :]
