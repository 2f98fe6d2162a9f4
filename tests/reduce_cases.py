"""Operands, exact references and checks of the reduction, slab-sum and state-update tests
(test_reduce_host.py on the CPU, test_gpu_reduce.py and test_gpu_update_state.py on the GPU).
Nothing here touches the GPU.

Vectors are raw limbs of shape (words, n); the number under test is the limb sum, a dyadic
rational, so every reference is exact: limbs become Python integers times a power of two
(gemm_cases.ints) and a result is an (I, e) pair, the integer I times 2^e.

Operand classes
  exact    every partial sum in any order is representable, so whatever the order of a kernel's
           sums the result must equal the exact one (compared as values: the sum of the limbs the
           device returns against the exact integer).  Leading limbs are nonzero integers of
           magnitude at most amax(n) < 2^18 with n amax^2 < 2^50; the trailing limbs of `a` are
           integers of magnitude 1 .. 8 times 2^-80, 2^-140 and 2^-190; `b` has one limb, so every
           product is exact.  A dropped, doubled or misplaced element changes the value.
  generic  full-width random limbs, element 2m+1 the negative of element 2m up to a relative
           2^-20, so that sum a b is about 1e-6 sum |a b|; compared against the exact sum with
           the componentwise a-priori bound below.
  extreme  (max, min, max-abs) values of magnitude below 1 with the extreme of magnitude 3 at a
           chosen position and runner-ups elsewhere that equal it in every limb but the last
           (words 1: the neighbouring double), so a comparison that looks at the leading limbs
           alone picks a wrong element; the result must be the extreme bitwise.

Bound.  A sum of n terms t_i in any order, every operation with relative error at most u, is
within ((1 + u)^(n+1) - 1) sum |t_i| <= (n + 2) u sum |t_i| of the exact one for n u < 1/4 (a
product or the pair of sums of a dot-of-sums term costs the roundings that the missing additions
of a tree leave free).  u = gemm_cases.EPS[words], the unit of the product tests, which at
double-double and quad-double already holds the constants of the multi-word operators; the factor
in front is the product bound's, SLACK = 1.  For a dot of sums the terms are bounded by
(|a| + |da|) (|b| + |db|): a multi-word sum is accurate relative to |a| + |da|, not to |a + da|.
"""
import numpy as np

import gemm_cases as gc

EPS = gc.EPS
SLACK = 1.0          # the factor in front of (K + extra) u in gemm_cases.bound
WORDS = (1, 2, 4)
RED_G = 256
# vec_reduce: threads and elements per thread and sweep
NT = {1: 1024, 2: 256, 4: 256}
U = {1: 4, 2: 2, 4: 1}
LIMB_EXP = (0, -80, -140, -190)
NAN_PAYLOAD = np.array([0x7FF8C0DEC0DEC0DE], dtype=np.uint64).view(np.float64)[0]


def rng(seed, *salt):
    return np.random.default_rng([int(seed)] + [int(s) for s in salt])


def amax(n, parts=1):
    """largest leading magnitude of the exact class at length n: n (parts amax)^2 < 2^50"""
    import math
    return max(1, min(2 ** 18 - 1, math.isqrt((2 ** 50 - 1) // int(n)) // parts))


def _nonzero_ints(r, n, m):
    v = r.integers(1, m + 1, size=n).astype(np.float64)
    return v * np.where(r.integers(0, 2, size=n) == 1, 1.0, -1.0)


def exact_vector(n, words, seed, m=None, trailing=True, mult=1.0):
    """limbs (words, n) of the exact class: leading integers of magnitude 1 .. m (multiples of
    `mult`), trailing limbs small integers times 2^LIMB_EXP[q] (or zero)"""
    r = rng(seed, n, words, 1)
    m = amax(n) if m is None else m
    v = np.zeros((words, n))
    v[0] = _nonzero_ints(r, n, max(1, int(m // mult))) * mult
    if trailing:
        for q in range(1, words):
            v[q] = _nonzero_ints(r, n, 8) * mult * 2.0 ** LIMB_EXP[q if words == 4 else 1]
    return v


def exact_pair(n, words, seed, parts=1):
    """(a, b) of the exact class for a dot product of length n (parts = 2: for a dot of sums)"""
    m = amax(n, parts)
    return exact_vector(n, words, seed, m), exact_vector(n, words, seed + 1, m, trailing=False)


_generic = {}


def generic_vector(n, words, seed, cancel=True):
    """limbs (words, n): every limb random at its natural magnitude, no zero entry, normalised;
    with `cancel` element 2m+1 = -(1 + r 2^-20) element 2m and an unpaired last one scaled 2^-20
    (computed once per argument set; the caller gets a copy)"""
    key = (n, words, seed, cancel)
    if key not in _generic:
        _generic[key] = _generic_vector(n, words, seed, cancel)
    return _generic[key].copy()


def _generic_vector(n, words, seed, cancel):
    r = rng(seed, n, words, 2)
    terms = []
    for t in range(words):
        u = r.uniform(-1.0, 1.0, size=n)
        if t == 0:
            u = np.where(u >= 0, 1.0, -1.0) * (0.5 + 0.5 * np.abs(u))
        terms.append(u * 2.0 ** (-53 * t))
    if cancel and n >= 2:
        odd = np.arange(1, n, 2)
        for t in terms:
            t[odd] = -t[odd - 1]
        extra = np.zeros(n)
        extra[odd] = -terms[0][odd - 1] * r.uniform(-1.0, 1.0, size=len(odd)) * 2.0 ** -20
        terms.append(extra)
        terms.sort(key=lambda x: -np.max(np.abs(x)))
        if n % 2:
            for t in terms:
                t[n - 1] *= 2.0 ** -20
    return gc.renorm(terms, words)


def generic_pair(n, words, seed):
    """(a, b): a cancels pairwise, b repeats pairwise, so sum a b ~ 2^-20 sum |a b|"""
    a = generic_vector(n, words, seed)
    b = generic_vector(n, words, seed + 1, cancel=False)
    if n >= 2:
        odd = np.arange(1, n, 2)
        b[:, odd] = b[:, odd - 1]
    return a, b


# ---- exact arithmetic on (I, e) -----------------------------------------------------------------
def ints(v):
    """limbs (words, n) (or (words,)) -> (object array of n Python integers, e)"""
    v = np.asarray(v, dtype=np.float64)
    if v.ndim == 1:
        v = v[:, None]
    I, e = gc.ints(v[:, None, :])
    return I[0], e


def add(x, y):
    (X, ex), (Y, ey) = x, y
    e = min(ex, ey)
    return (X << (ex - e)) + (Y << (ey - e)), e


def scale(x, c):
    """c x for a float c"""
    ci, ec = gc.ints(np.array([float(c)]))
    return x[0] * int(ci[0]), x[1] + ec


def same(x, y):
    (X, ex), (Y, ey) = x, y
    e = min(ex, ey)
    return bool(np.all((X << (ex - e)) == (Y << (ey - e))))


def dot_ints(a, b, da=None, db=None):
    """exact sum (a + da) (b + db) as (I, e) of one number"""
    A, B = ints(a), ints(b)
    if da is not None:
        A, B = add(A, ints(da)), add(B, ints(db))
    return np.array([(A[0] * B[0]).sum()], dtype=object), A[1] + B[1]


def sum_ints(v):
    I, e = ints(v)
    return np.array([I.sum()], dtype=object), e


def colsum_ints(sl):
    """slabs (words, cnt, n) -> the exact column sums (n integers, e)"""
    I, e = gc.ints(np.asarray(sl, dtype=np.float64))
    return I.sum(axis=0), e


def matvec_ints(Q, r):
    """exact Q r for a float matrix Q and r = (I, e)"""
    Qi, eq = gc.ints(np.asarray(Q, dtype=np.float64))
    return Qi @ r[0], eq + r[1]


def lead(v):
    return np.abs(np.asarray(v, dtype=np.float64)[0])


def dot_bound(words, a, b, da=None, db=None):
    ta = lead(a) + (0.0 if da is None else lead(da))
    tb = lead(b) + (0.0 if db is None else lead(db))
    return SLACK * (ta.size + 2) * EPS[words] * float(np.sum(ta * tb))


def sum_bound(words, v, extra_terms=0):
    v = np.asarray(v, dtype=np.float64)
    return SLACK * (v.shape[-1] + extra_terms + 2) * EPS[words] * float(np.sum(lead(v)))


# ---- the checks the GPU tests use ---------------------------------------------------------------
def value_equal(got, ref):
    """the limb sums of `got` (words, ...) equal the exact (I, e), entry by entry; no NaN"""
    got = np.asarray(got, dtype=np.float64)
    if not np.all(np.isfinite(got)):
        return False
    return same(ints(got), ref)


def ratio(got, ref, bnd):
    """max |got - ref| / bound (gemm_cases.ratio: exact differences, mpmath decides); got limbs
    (words,) or (words, n), ref (I, e) with n integers, bnd a float or n floats"""
    got = np.asarray(got, dtype=np.float64)
    if got.ndim == 1:
        got = got[:, None]
    n = got.shape[1]
    bnd = np.broadcast_to(np.asarray(bnd, dtype=np.float64), (n,))
    return gc.ratio(got[:, None, :], (np.asarray(ref[0], dtype=object).reshape(1, n), ref[1]),
                    bnd.reshape(1, n))


def judge(kind, got, ref, bnd):
    """(passes, figure): the exact class must be the reference as a value (figure 0 or inf), any
    other class within the bound (figure = error / bound)"""
    if kind == "exact":
        ok = value_equal(got, ref)
        return ok, 0.0 if ok else float("inf")
    if not np.all(np.isfinite(np.asarray(got, dtype=np.float64))):
        return False, float("inf")
    r = ratio(got, ref, bnd)
    return r <= 1.0, r


def to_limbs(ref, words):
    """the canonical limbs (words, n) of an exact (I, e): what a correct kernel would return where
    the value fits the width"""
    return gc.split(gc.to_mpf(*ref), words).reshape(words, -1)


def bitwise(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return x.shape == y.shape and bool(np.all(x.view(np.uint64) == y.view(np.uint64)))


def is_nan(got):
    return bool(np.isnan(np.asarray(got, dtype=np.float64).reshape(-1)[0]))


# ---- extreme class ------------------------------------------------------------------------------
def extreme_limbs(words, runner=False):
    """the extreme 3 + 2^-60 + 2^-120 + 2^-180 cut to `words` limbs; the runner-up has the last
    limb halved (words 1: the double below 3)"""
    full = np.array([3.0, 2.0 ** -60, 2.0 ** -120, 2.0 ** -180])[:words].copy()
    if runner:
        full[-1] = np.nextafter(3.0, 0.0) if words == 1 else full[-1] * 0.5
    return full


def positions(n, words, chunk=None):
    """the structurally distinct positions of an extreme in a vector of n: the ends, the thread
    count and sweep of vec_reduce, the wave of the folds, a flat_reduce chunk's first and last"""
    nt, u = NT[words], U[words]
    p = {0, n - 1, nt - 1, nt, u * nt - 1, u * nt, 63, 64, 65}
    if chunk:
        p |= {chunk - 1, chunk, 2 * chunk - 1}
    return sorted(q for q in p if 0 <= q < n)


def extreme_vector(n, words, seed, pos, op, nan=False):
    """(vector, expected limbs) for op in max / min / maxabs: magnitudes below 1 everywhere, the
    extreme at `pos` (max: +E, min: -E, maxabs: -E, and a +runner-up elsewhere so that max alone
    is wrong), runner-ups at up to four other positions; with `nan` a NaN replaces the extreme
    and the expected result is NaN"""
    v = generic_vector(n, words, seed, cancel=False) * 0.5
    E, R = extreme_limbs(words), extreme_limbs(words, runner=True)
    sgn = 1.0 if op == "max" else -1.0
    others = [q for q in (0, n - 1, pos - 1, pos + 1, (pos + 64) % n, n // 2) if 0 <= q < n and q != pos]
    for k, q in enumerate(dict.fromkeys(others)):
        v[:, q] = (sgn if (op != "maxabs" or k % 2) else 1.0) * R
    v[:, pos] = sgn * E
    want = E if op in ("max", "maxabs") else -E
    if nan:
        v[0, pos] = np.nan
        want = np.full(words, np.nan)
    return v, want


# ---- the documented order of scalar_kernel's fp64 fold ------------------------------------------
def fold_sum_f64(v):
    """lane l takes l, l + 64, ... in order (a lane without elements: 0), then the xor butterfly
    32 .. 1; every step an fp64 addition"""
    v = np.asarray(v, dtype=np.float64)
    acc = np.zeros(64)
    for l in range(min(64, v.size)):
        s = v[l]
        for i in range(l + 64, v.size, 64):
            s = s + v[i]
        acc[l] = s
    o = 32
    while o:
        acc = acc + acc[np.arange(64) ^ o]
        o >>= 1
    return acc[0]


def flat_chunk(n, g=RED_G):
    return -(-n // g)
