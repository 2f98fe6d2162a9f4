"""Instances, operands, exact references, bounds and checks of the low-rank operator, block
kernel and cluster-solve tests (test_oper_host.py on the CPU, test_gpu_operators.py and
test_gpu_cl_solve.py on the GPU).  Nothing here touches the GPU.

Instances are built directly as oracle ``Cluster(A, B, c, H)`` objects: nothing is factorised, so
sample counts, B, c and b are free.  Three kinds, so that every route is the library's own choice:
  trivial  m = L = rank = 1, delta 1, 63, 64, 65, 129 (N = 1, 6, 7, 8, 130): colsum_rhs; at fp64
           the fused weighted A, at multi-word scale_cols with delta K = 16770 > 64 x 256 threads
  uniform  two equal clusters, delta = 67, N = 7: the strip chain's TRACE form at fp64
  general  eight clusters, m in {1, 2, 3}, L in {1, 2, 3}, ranks 0 .. 3 (rank-0 first and last
           samples), block sizes 1, 31, 33, 32, 129, 3, 15, 64, 128, 65, 127, 129, 63 with the m > 1
           blocks a middle subset, 266 local tuples with cluster boundaries at 196 and 266:
           colsum_dot + tuple_aggregate, scale_cols (rank > 1: column != sample; m >= 2: the 1/2)
Column counts K mod 4 take 0, 1, 2 and 3 in the trivial and in the general kind.

Operands are raw limbs, (words, n) for the flat block arena (blocks column-major, in order) and
for the tuples.  Classes as in reduce_cases.py / gemm_cases.py:
  exact    V, lambda and every coefficient one-limb integers (lambda of both signs), Z or a small
           integers with trailing limbs of magnitude 1 .. 8 at 2^-80 / 2^-140 / 2^-190, capped
           (caps_ok) so that every partial sum in any order is representable: the result must
           equal the exact integer as a value.
  generic  full-width random limbs; rows 2q, 2q+1 and columns 2q, 2q+1 of V equal, columns of Z
           and the lambdas pairwise cancelling to 2^-20, a pairwise equal over the samples: Z
           non-symmetric, |result| << sum |terms|.  Compared componentwise with the bound below.

References are exact: limbs become Python integers times a power of two (gemm_cases.ints), and
``rhs_eval`` / ``weighted_eval`` restate trace_A and compute_weighted_A of oracle/mpmp_oracle.py
on them (test_oper_host.py shows that they equal the oracle's own functions at 256 bits on these
instances, and runs the same code in float64 as the fp64 numpy restatement).

Bound: (ops + 2) u sum |terms| (reduce_cases.py, SLACK = 1), ops the operations a term passes
through, u = EPS[words].
  RHS       rhs_t = -d_t - sum_l sum_{p in k} lambda_p v_p^T Z_rs v_p: a term of block l passes
            through delta_l additions in U = Z V, delta_l in the column dot, the n_t columns
            aggregated into the tuple, and the lambda and coefficient products:
            ops = 2 delta_l + n_t + 2; d_t itself through n_t + 2.
  WEIGHTED  out_ij = base_ij + sum_p V_ip w_p V_jp, w_p = a_k(p) lambda_p (1/2): K additions and
            the scale products (a lambda, the 1/2, V w: 3; the fused scaled GEMM forms
            (a lambda) V: 2): ops = K + 3 (K + 2 fused); base_ij is one more term.
  LIN       2 u (|A| + |B|) per element (one product with a unit coefficient, one addition).
"""
import numpy as np

import gemm_cases as gc
import reduce_cases as rc

EPS = rc.EPS
SLACK = rc.SLACK
WORDS = rc.WORDS
KINDS = ("trivial", "uniform", "general")
CLASSES = ("exact", "generic")
N_Y = 3
NAN = rc.NAN_PAYLOAD
# a second payload, so that a guard that was copied is told from one that was left
NAN2 = np.array([0x7FF8BADDBADDBADD], dtype=np.uint64).view(np.float64)[0]
# routes reported by clrsdp_apply_operator
ROUTE_RHS = {("trivial", 1): 1, ("trivial", 2): 1, ("trivial", 4): 1,
             ("uniform", 1): 0, ("uniform", 2): 1, ("uniform", 4): 1,
             ("general", 1): 2, ("general", 2): 2, ("general", 4): 2}
ROUTE_WEIGHTED = {("trivial", 1): 0, ("trivial", 2): 1, ("trivial", 4): 1,
                  ("uniform", 1): 0, ("uniform", 2): 1, ("uniform", 4): 1,
                  ("general", 1): 1, ("general", 2): 1, ("general", 4): 1}


def spec(kind):
    """per cluster: m, the deltas of its blocks, the sample count N and ranks[l][k]"""
    one = lambda d, n: dict(m=1, deltas=[d], N=n, ranks=[[1] * n])
    if kind == "trivial":
        return [one(1, 1), one(63, 6), one(64, 7), one(65, 8), one(129, 130)]
    if kind == "uniform":
        return [one(67, 7), one(67, 7)]
    assert kind == "general"
    return [
        one(1, 1),
        dict(m=1, deltas=[31, 33], N=5, ranks=[[0, 2, 1, 3, 0], [1, 0, 2, 0, 1]]),
        dict(m=2, deltas=[16], N=3, ranks=[[2, 1, 2]]),
        dict(m=3, deltas=[43, 1, 5], N=4, ranks=[[1, 0, 1, 1], [0, 3, 0, 0], [2, 1, 0, 1]]),
        dict(m=2, deltas=[32, 64], N=7, ranks=[[1] * 7, [1, 2, 0, 1, 1, 0, 2]]),
        dict(m=1, deltas=[65, 127], N=6, ranks=[[1] * 6, [0, 1, 1, 3, 1, 0]]),
        dict(m=1, deltas=[129], N=130, ranks=[[2] + [1] * 127 + [0, 1]]),
        one(63, 70),
    ]


class Layout:
    """offsets of a kind: blocks[(j, l)] = (offset in the block arena, n, delta, K, m),
    x_off[j], the sample of every column and the rank sums"""

    def __init__(self, kind):
        self.kind, self.spec = kind, spec(kind)
        self.blocks, self.x_off, self.ks, self.rsum = {}, [], {}, {}
        off = xo = 0
        for j, c in enumerate(self.spec):
            self.x_off.append(xo)
            xo += c["m"] * (c["m"] + 1) // 2 * c["N"]
            for l, d in enumerate(c["deltas"]):
                rk = c["ranks"][l]
                assert len(rk) == c["N"] and sum(rk) > 0
                n = c["m"] * d
                self.blocks[(j, l)] = (off, n, d, sum(rk), c["m"])
                self.ks[(j, l)] = np.repeat(np.arange(c["N"]), rk)
                self.rsum[(j, l)] = np.concatenate([[0], np.cumsum(rk)])
                off += n * n
        self.n_blk, self.n_x, self.J = off, xo, len(self.spec)
        self.order = sorted(self.blocks, key=lambda q: self.blocks[q][0])

    def block(self, flat, j, l):
        """the (n, n) view of block (j, l) of a flat arena (any dtype)"""
        off, n = self.blocks[(j, l)][:2]
        return flat[off:off + n * n].reshape(n, n, order="F")

    def sizes(self):
        return [self.blocks[q][1] for q in self.order]

    def m_of(self):
        return [self.blocks[q][4] for q in self.order]

    def unread_mask(self, upper):
        """flat mask of the off-diagonal sub-blocks an operator never reads on blocks with m > 1:
        ``upper`` (RHS: Z[r, s] with r < s, block rows r and columns s) or the lower ones
        (WEIGHTED: the base below the block diagonal)"""
        mask = np.zeros(self.n_blk, dtype=bool)
        for (j, l), (off, n, d, K, m) in self.blocks.items():
            M = np.zeros((n, n), dtype=bool)
            for r in range(m):
                for s in range(m):
                    if (r < s) if upper else (r > s):
                        M[r * d:(r + 1) * d, s * d:(s + 1) * d] = True
            mask[off:off + n * n] = M.reshape(-1, order="F")
        return mask


_layouts = {}


def layout(kind):
    if kind not in _layouts:
        _layouts[kind] = Layout(kind)
    return _layouts[kind]


# ---- operands -----------------------------------------------------------------------------------
def _ints_pm(r, shape, m):
    return r.integers(1, m + 1, size=shape).astype(np.float64) * np.where(r.integers(0, 2, size=shape) == 1, 1.0, -1.0)


def _trailing(r, v, words):
    """limbs (words, ...) with leading v and trailing integers 1 .. 8 at 2^LIMB_EXP"""
    out = np.zeros((words,) + v.shape)
    out[0] = v
    for q in range(1, words):
        out[q] = _ints_pm(r, v.shape, 8) * 2.0 ** rc.LIMB_EXP[q if words == 4 else 1]
    return out


def _generic(r, shape, words, scale=1.0):
    """full-width random limbs (words, ...), leading magnitude in [1/2, 1) scale, no zero"""
    terms = []
    for t in range(words):
        u = r.uniform(-1.0, 1.0, size=shape)
        if t == 0:
            u = np.where(u >= 0, 1.0, -1.0) * (0.5 + 0.5 * np.abs(u))
        terms.append(u * scale * 2.0 ** (-53 * t))
    return gc.renorm(terms, words)


def _pair_cancel(r, x, axis, words):
    """entry 2q+1 along `axis` := -(1 + r 2^-20) entry 2q (an unpaired last one scaled 2^-20)"""
    x = np.moveaxis(x.copy(), axis + 1, 1)            # (words, n, ...)
    n = x.shape[1]
    odd = np.arange(1, n, 2)
    terms = [x[q].copy() for q in range(words)]
    for t in terms:
        t[odd] = -t[odd - 1]
    extra = np.zeros_like(terms[0])
    extra[odd] = -terms[0][odd - 1] * r.uniform(-1.0, 1.0, size=extra[odd].shape) * 2.0 ** -20
    terms.append(extra)
    if n % 2:
        for t in terms:
            t[n - 1] *= 2.0 ** -20
    terms.sort(key=lambda v: -np.max(np.abs(v)))
    return np.moveaxis(gc.renorm(terms, words), 1, axis + 1)


class Instance:
    """one (kind, class, words): the constraint data as limbs and as oracle Clusters"""

    def __init__(self, kind, cls, words, seed=7):
        self.kind, self.cls, self.words = kind, cls, words
        self.lay = lay = layout(kind)
        r = rc.rng(seed, KINDS.index(kind), CLASSES.index(cls), words)
        self.V, self.lam = {}, {}
        for (j, l) in lay.order:
            _, n, d, K, m = lay.blocks[(j, l)]
            if cls == "exact":
                V = np.zeros((words, d, K))
                V[0] = _ints_pm(r, (d, K), 2)
                lam = np.zeros((words, K))
                lam[0] = _ints_pm(r, K, 3)
                lam[0, ::2] = -np.abs(lam[0, ::2])      # both signs whatever the draw
                lam[0, 1::2] = np.abs(lam[0, 1::2])
            else:
                h, hk = (d + 1) // 2, (K + 1) // 2
                base = _generic(r, (h, hk), words)
                V = np.repeat(np.repeat(base, 2, axis=1), 2, axis=2)[:, :d, :K]
                lam = _pair_cancel(r, _generic(r, (K,), words), 0, words)
            self.V[(j, l)], self.lam[(j, l)] = V, lam
        dims = [c["m"] * (c["m"] + 1) // 2 * c["N"] for c in lay.spec]
        self.B = [_ints_pm(r, (D, N_Y), 3) for D in dims]
        self.c = [_ints_pm(r, D, 5) for D in dims]
        self.b = _ints_pm(r, N_Y, 5)
        self._ints = None

    def ints(self):
        """V and lambda of every block as object integers at one exponent each: (Vi, ev, li, el)"""
        if self._ints is None:
            w, order = self.words, self.lay.order
            Vf = np.concatenate([self.V[q].reshape(w, -1) for q in order], axis=1)
            lf = np.concatenate([self.lam[q] for q in order], axis=1)
            (VI, ev), (lI, el) = rc.ints(Vf), rc.ints(lf)
            Vi, li, vo, lo = {}, {}, 0, 0
            for q in order:
                d, K = self.V[q].shape[1:]
                Vi[q] = VI[vo:vo + d * K].reshape(d, K)
                li[q] = lI[lo:lo + K]
                vo, lo = vo + d * K, lo + K
            self._ints = (Vi, ev, li, el)
        return self._ints

    def data(self, q, exact):
        """(V, lambda) of block q: object integers (exponents from ints()) or float64"""
        if exact:
            Vi, _, li, _ = self.ints()
            return Vi[q], li[q]
        return self.V[q].sum(axis=0), self.lam[q].sum(axis=0)

    def values(self, limbs):
        """what a Cluster holds: floats at one word (or one-limb data), mpf limb sums above"""
        if self.words == 1 or not np.any(limbs[1:]):
            return limbs[0].copy()
        return gc.limb_sum(limbs.reshape(self.words, 1, -1))[0].reshape(limbs.shape[1:])

    def clusters(self):
        """the instance as the package's Cluster(A, B, c, H) objects (the oracle reads the same
        attributes)"""
        import _clrsdp_pkg
        Cluster = _clrsdp_pkg.load().instance.Cluster
        lay, out = self.lay, []
        for j, c in enumerate(lay.spec):
            A, H = [], []
            for l in range(len(c["deltas"])):
                V, lam = self.values(self.V[(j, l)]), self.values(self.lam[(j, l)])
                rs = lay.rsum[(j, l)]
                A.append([[V[:, p] for p in range(rs[k], rs[k + 1])] for k in range(c["N"])])
                H.append([[lam[p] for p in range(rs[k], rs[k + 1])] for k in range(c["N"])])
            out.append(Cluster(A, self.B[j].copy(), self.c[j].copy(), H))
        return out

    # -- operands of the two operators ---------------------------------------------------------
    def blocks(self, salt, zmax=64, cancel=True):
        """a flat block operand (words, n_blk): non-symmetric, every block unrelated"""
        lay, words = self.lay, self.words
        r = rc.rng(11, salt, KINDS.index(self.kind), CLASSES.index(self.cls), words)
        out = np.zeros((words, lay.n_blk))
        for q in lay.order:
            off, n = lay.blocks[q][:2]
            if self.cls == "exact":
                Z = _trailing(r, _ints_pm(r, (n, n), zmax), words)
            else:
                Z = _generic(r, (n, n), words)
                if cancel:                                # columns pair up inside every delta block
                    d = lay.blocks[q][2]
                    for s in range(lay.blocks[q][4]):
                        Z[:, :, s * d:(s + 1) * d] = _pair_cancel(r, Z[:, :, s * d:(s + 1) * d], 1, words)
            out[:, off:off + n * n] = np.stack([Z[w].reshape(-1, order="F") for w in range(words)])
        return out

    def tuples(self, salt, amax=16, pairs=False):
        """a tuple operand (words, n_x); `pairs`: equal over the samples 2q, 2q+1 of a cluster"""
        lay, words = self.lay, self.words
        r = rc.rng(13, salt, KINDS.index(self.kind), CLASSES.index(self.cls), words)
        if self.cls == "exact":
            return _trailing(r, _ints_pm(r, lay.n_x, amax), words)
        v = _generic(r, (lay.n_x,), words)
        if pairs:
            for j, c in enumerate(lay.spec):
                N = c["N"]
                for rs in range(c["m"] * (c["m"] + 1) // 2):
                    o = lay.x_off[j] + rs * N
                    odd = np.arange(1, N, 2)
                    v[:, o + odd] = v[:, o + odd - 1]
        return v


_inst = {}


def instance(kind, cls, words):
    key = (kind, cls, words)
    if key not in _inst:
        _inst[key] = Instance(kind, cls, words)
    return _inst[key]


# ---- the operators restated (object integers: the exact reference; float64: the fp64 model) ------
def _as(x, exact):
    """limbs (words, ...) -> (array, e): object integers times 2^e, or the float64 limb sums"""
    x = np.asarray(x, dtype=np.float64)
    if exact:
        I, e = rc.ints(x.reshape(x.shape[0], -1))
        return I.reshape(x.shape[1:]), e
    return x.sum(axis=0), 0


def _pairs(m):
    return [(r, s) for r in range(m) for s in range(r + 1)]


def rhs_eval(inst, Z, d, exact=True, mut=None):
    """rhs = -d - Tr(A_* Z) for a flat Z taken as given (trace_A, MPMP.jl:1517-1584: tuple
    (r, s <= r, k) takes lambda_p v_p^T Z[r, s] v_p of the columns p of sample k, block rows r and
    columns s; then MPMP.jl:1733-1739).  Returns ((values (n_x,), e), bound (n_x,)); the bound is
    u (sum_l (2 delta_l + n_t + 4) sum |terms_l| + (n_t + 4) |d_t|).  `mut` names a way to be
    wrong (test_oper_host.py)."""
    lay = inst.lay
    Zi, ez = _as(Z, exact)
    di, ed = _as(d, exact)
    zero = 0 if exact else 0.0
    res = np.full(lay.n_x, zero, dtype=object if exact else np.float64)
    wsum, asum, ncols = np.zeros(lay.n_x), np.zeros(lay.n_x), np.zeros(lay.n_x)
    absZ = np.abs(np.asarray(Z, dtype=np.float64)[0])
    for q in lay.order:
        j, l = q
        _, n, dl, K, m = lay.blocks[q]
        N = lay.spec[j]["N"]
        V, lam = inst.data(q, exact)
        aV, aL = np.abs(inst.V[q][0]), np.abs(inst.lam[q][0])
        ks, rsum = lay.ks[q], lay.rsum[q]
        Zb, aZb = lay.block(Zi, j, l), lay.block(absZ, j, l)
        for r, s in _pairs(m):
            rr, ss = (s, r) if mut == "swap_rs" else (r, s)
            U = Zb[rr * dl:(rr + 1) * dl, ss * dl:(ss + 1) * dl] @ V       # U = Z[r, s] V
            rows = min(dl, 64) if mut == "lane64" else dl
            val = (U[:rows] * V[:rows]).sum(axis=0)                         # one wave per column
            if mut == "drop_last_col" and K % 4:
                val[K - 1] = zero
            off = lay.x_off[j] + (s + r * (r + 1) // 2) * N
            for k in range(N):
                lo, hi = rsum[k], rsum[k + 1]
                if mut == "ranksum_off" and hi == lo and lo < K:
                    hi = lo + 1                     # a rank-0 sample takes its neighbour's column
                for p in range(lo, hi):
                    res[off + k] = res[off + k] + lam[p] * val[p]
            aval = ((aZb[r * dl:(r + 1) * dl, s * dl:(s + 1) * dl] @ aV) * aV).sum(axis=0) * aL
            np.add.at(asum, off + ks, aval)
            np.add.at(wsum, off + ks, (2 * dl + 2) * aval)
            np.add.at(ncols, off + ks, 1.0)
    ad = np.abs(np.asarray(d, dtype=np.float64)[0])
    bnd = SLACK * EPS[inst.words] * (wsum + (ncols + 2) * asum + (ncols + 4) * ad)
    if not exact:
        return (-di - res, 0), bnd
    _, ev, _, el = inst.ints()
    et = ez + 2 * ev + el
    e = min(et, ed)
    return (-(di << (ed - e)) - (res << (et - e)), e), bnd


def weighted_eval(inst, a, base, exact=True, mut=None, fused=False):
    """base + sum_i a_i A_i as weighted_A forms it (compute_weighted_A, MPMP.jl:1621-1678: block
    (s, r), s <= r, is V diag(w) V^T, w_p = a_(r, s, k(p)) lambda_p, halved off the block diagonal;
    a block with m > 1 is its upper triangle mirrored).  Returns ((flat values, e), flat bound);
    the bound is (K + 3 + 2) u (sum |terms| + |base|), K + 2 + 2 for the fused scaled GEMM."""
    lay = inst.lay
    ai, ea = _as(a, exact)
    Bi, eb = _as(base, exact)
    absB = np.abs(np.asarray(base, dtype=np.float64)[0])
    absa = np.abs(np.asarray(a, dtype=np.float64)[0])
    out = np.zeros(lay.n_blk, dtype=object if exact else np.float64)
    bnd = np.zeros(lay.n_blk)
    et = e = 0
    if exact:
        _, ev, _, el = inst.ints()
        et = ea + el + 2 * ev - 1                              # (every weight doubled: the halves)
        e = min(et, eb)
    for q in lay.order:
        j, l = q
        off, n, dl, K, m = lay.blocks[q]
        N = lay.spec[j]["N"]
        V, lam = inst.data(q, exact)
        aV, aL = np.abs(inst.V[q][0]), np.abs(inst.lam[q][0])
        ks = lay.ks[q]
        M = np.zeros((n, n), dtype=out.dtype)
        T = np.zeros((n, n))
        Bb, aBb = lay.block(Bi, j, l), lay.block(absB, j, l)
        for r, s in _pairs(m):
            o = lay.x_off[j] + (s + r * (r + 1) // 2) * N
            smp = np.minimum(np.arange(K), N - 1) if mut == "col_as_sample" else ks
            w = ai[o + smp] * lam
            half = r != s and mut != "half"
            if exact:
                w = w * (1 if half else 2)
            elif half:
                w = w * 0.5
            Q = (V * w) @ V.T
            sl = (slice(s * dl, (s + 1) * dl), slice(r * dl, (r + 1) * dl))
            M[sl] = (Q << (et - e)) + (Bb[sl] << (eb - e)) if exact else Q + Bb[sl]
            aw = absa[o + ks] * aL * (0.5 if r != s else 1.0)
            T[sl] = (K + (2 if fused else 3) + 2) * ((aV * aw) @ aV.T + aBb[sl])
        if m != 1:                                             # Symmetric(.): the upper triangle
            iu = np.triu_indices(n, 1)
            M.T[iu] = M[iu]
            T.T[iu] = T[iu]
        out[off:off + n * n] = M.reshape(-1, order="F")
        bnd[off:off + n * n] = T.reshape(-1, order="F")
    return (out, e), SLACK * EPS[inst.words] * bnd


class _Abs:
    """an instance with |V| and |lambda| in one limb (for sums of absolute terms)"""

    def __init__(self, inst):
        self.lay, self.words = inst.lay, 1
        self.V = {q: np.abs(v[:1]) for q, v in inst.V.items()}
        self.lam = {q: np.abs(v[:1]) for q, v in inst.lam.items()}

    def data(self, q, exact):
        return self.V[q][0], self.lam[q][0]


def abs_sums(inst, Z, d, a, base, plane=0, scale=1.0):
    """(max over the tuples of |d| + sum |terms| of RHS, max over the entries of |base| + sum
    |terms| of WEIGHTED, without the halves) of limb plane `plane` times `scale`, in float64: the
    restatements evaluated on absolute values"""
    ab = _Abs(inst)
    pl = lambda x: np.abs(np.asarray(x, dtype=np.float64)[plane:plane + 1]) * scale
    (r1, _), _ = rhs_eval(ab, pl(Z), pl(d), exact=False)
    (r2, _), _ = weighted_eval(ab, pl(a), pl(base), exact=False, mut="half")
    return float(np.max(np.abs(r1))), float(np.max(np.abs(r2)))


def caps_ok(inst, Z, d, a, base):
    """exact class: limb plane by limb plane (integers at 2^0, 2^-80, 2^-140, 2^-190; V and lambda
    have one limb), sum |terms| of every result of both operators stays below 2^49, so whatever
    the order every partial sum is an integer of fewer than 50 bits per plane: representable at
    every width (at fp64: below 2^53), the planes at least 50 bits apart"""
    w = inst.words
    for q in inst.lay.order:
        if np.any(inst.V[q][1:]) or np.any(inst.lam[q][1:]):
            return False
    for p in range(w):
        sc = 2.0 ** -rc.LIMB_EXP[p if w == 4 else min(p, 1)]
        for x in (Z, d, a, base):
            v = np.asarray(x)[p] * sc
            if not np.all(v == np.round(v)):
                return False
        if max(abs_sums(inst, Z, d, a, base, p, sc)) >= 2.0 ** 49:
            return False
    return True


# ---- checks the GPU tests use -------------------------------------------------------------------
def judge(cls, got, ref, bnd, mask=None):
    """(passes, error / bound): exact class equal as a value, generic within the bound; entries
    outside `mask` do not count"""
    got = np.asarray(got, dtype=np.float64)
    I, e = ref
    bnd = np.broadcast_to(np.asarray(bnd, dtype=np.float64), I.shape)
    if mask is not None:
        got, I, bnd = got[:, mask], I[mask], bnd[mask]
    if not np.all(np.isfinite(got)):
        return False, float("inf")
    if cls == "exact":
        ok = rc.same(rc.ints(got), (I, e))
        return ok, 0.0 if ok else float("inf")
    fig = rc.ratio(got, (I, e), bnd)
    return fig <= 1.0, fig


def mirrored_bitwise(lay, got):
    """every block with m > 1 of a flat result (words, n_blk) is bitwise symmetric"""
    for q in lay.order:
        off, n, _, _, m = lay.blocks[q]
        if m > 1:
            for w in range(got.shape[0]):
                B = got[w, off:off + n * n].reshape(n, n, order="F")
                if not rc.bitwise(B, np.ascontiguousarray(B.T)):
                    return False
    return True


def all_bitwise_symmetric(lay, got, only_m=False):
    for q in lay.order:
        off, n, _, _, m = lay.blocks[q]
        if only_m and m == 1:
            continue
        for w in range(got.shape[0]):
            B = got[w, off:off + n * n].reshape(n, n, order="F")
            if not rc.bitwise(B, np.ascontiguousarray(B.T)):
                return False
    return True


def sym_expect(lay, X, mode, only_m, out0):
    """what sym(out, X, mode, only_m) must leave in an `out` that held out0: (limbs, None) for the
    modes that copy entries (1: the upper triangle mirrored, 2: the transpose; bitwise), (None,
    (I, e)) for mode 0 on dyadic input ((Z + Z^T) / 2 exactly, the diagonal copied); and the mask
    of the entries the launch may write"""
    words = X.shape[0]
    exp = np.array(out0, dtype=np.float64, copy=True)
    touched = np.zeros(lay.n_blk, dtype=bool)
    I, e = rc.ints(np.where(np.isfinite(X), X, 0.0))
    S = I.copy()
    for q in lay.order:
        off, n, _, _, m = lay.blocks[q]
        if only_m and m == 1:
            continue
        touched[off:off + n * n] = True
        Ib = I[off:off + n * n].reshape(n, n, order="F")
        S[off:off + n * n] = (Ib + Ib.T).reshape(-1, order="F")   # at exponent e - 1
        for w in range(words):
            B = X[w, off:off + n * n].reshape(n, n, order="F")
            R = np.triu(B) + np.triu(B, 1).T if mode == 1 else B.T
            exp[w, off:off + n * n] = R.reshape(-1, order="F")
    S[~touched] = 2 * I[~touched]
    return (exp, None, touched) if mode != 0 else (None, (S, e - 1), touched)


def lin_bound(words, A, B=None):
    """2 u (|A| + |B|) per element"""
    t = np.abs(np.asarray(A, dtype=np.float64)[0])
    if B is not None:
        t = t + np.abs(np.asarray(B, dtype=np.float64)[0])
    return 2 * EPS[words] * t


# ---- the cluster solve --------------------------------------------------------------------------
CL_BATCHES = ([1, 65, 256], [64, 129], [63, 128, 193, 255], [192])
CL_NY = (1, 2, 3, 4, 5, 31, 32, 33, 127, 128, 129, 160)


def cl_operands(Ds, ny, cls, seed=3):
    """per cluster L^-1 (lower triangular, NaN above the diagonal), W, rhs; dy.  exact: integers
    with L in {-1, 0, 1} (a few nonzeros per row beside a unit diagonal), W in {-1, 0, 1}, rhs and
    dy small, so every partial sum of t, the slabs, u and dx is an integer below 2^53 in any
    order; generic: random with pairwise-cancelling rhs"""
    r = rc.rng(seed, ny, len(Ds), CLASSES.index(cls), *Ds)
    Ls, Ws, rs = [], [], []
    for D in Ds:
        if cls == "exact":
            L = np.tril(r.integers(-1, 2, size=(D, D)).astype(np.float64), -1)
            L[np.diag_indices(D)] = np.where(r.integers(0, 2, size=D) == 1, 1.0, -1.0)
            W = r.integers(-1, 2, size=(D, ny)).astype(np.float64)
            rhs = _ints_pm(r, D, 4)
        else:
            L = np.tril(r.uniform(-1.0, 1.0, size=(D, D)))
            L[np.diag_indices(D)] = 1.0 + np.abs(np.diag(L))
            W = r.uniform(-1.0, 1.0, size=(D, ny))
            rhs = rc.generic_vector(D, 1, seed + D)[0]
        L[np.triu_indices(D, 1)] = NAN
        Ls.append(L)
        Ws.append(W)
        rs.append(rhs)
    dy = _ints_pm(r, ny, 4) if cls == "exact" else r.uniform(-1.0, 1.0, size=ny)
    return Ls, Ws, rs, dy


def cl_eval(Ls, Ws, rs, dy, exact=True, mut=None):
    """t_c = L_c rhs_c, slab (c, block) = W_c[rows of the block]^T t_c[rows] (zeros past D),
    u = t + W dy, dx = L^T u, with L the lower triangle: exact (I, e) values and the composed
    bounds, per cluster lists (t, slabs (nrb, ny), dx) and (bt, bs, bx):
      bt = (i + 1 + 2) u |L||rhs|              (row i: i + 1 terms)
      bs = |W|^T bt + (rows + 2) u |W|^T |t|   (bound(t) carried through W, then the sum's own)
      bu = bt + (ny + 1 + 2) u (|t| + |W||dy|)
      bx = |L|^T bu + (D - j + 2) u |L|^T |u|"""
    u1 = EPS[1]
    nrb = max(1, -(-max(L.shape[0] for L in Ls) // 64))
    out = []
    for L, W, rhs in zip(Ls, Ws, rs):
        D, ny = W.shape
        Lt = np.tril(np.where(np.isnan(L), 0.0, L))
        conv = (lambda x: _as(np.asarray(x, dtype=np.float64)[None], True)) if exact else (lambda x: (np.asarray(x, dtype=np.float64), 0))
        Li, eL = conv(Lt)
        Wi, eW = conv(W)
        ri, er = conv(rhs)
        yi, ey = conv(dy)
        t = Li @ ri
        et = eL + er
        aL, aW = np.abs(Lt), np.abs(W)
        at = aL @ np.abs(rhs)
        bt = (np.arange(D) + 3) * u1 * at
        slabs = np.zeros((nrb, ny), dtype=t.dtype)
        bs = np.zeros((nrb, ny))
        for rb in range(nrb):
            lo, hi = 64 * rb, min(64 * rb + 64, D)
            if lo >= D:
                continue
            rows = list(range(lo, hi))
            if mut == "skip_row64" and 64 in rows:
                rows.remove(64)
            cols = ny if mut != "w_col128" else min(ny, 128)
            slabs[rb, :cols] = Wi[rows, :cols].T @ t[rows]
            bs[rb] = aW[lo:hi].T @ bt[lo:hi] + (hi - lo + 2) * u1 * (aW[lo:hi].T @ at[lo:hi])
        Wy = Wi @ yi                                            # exponent eW + ey
        if exact:
            eu = min(et, eW + ey)
            uu = ((t << (et - eu)) if mut != "no_t" else 0) + (Wy << (eW + ey - eu))
        else:
            eu = 0
            uu = (t if mut != "no_t" else 0.0) + Wy
        au = at + aW @ np.abs(dy)
        bu = bt + (ny + 3) * u1 * au
        dx = Li.T @ uu
        bx = aL.T @ bu + (D - np.arange(D) + 2) * u1 * (aL.T @ au)
        out.append((((t, et), (slabs, et + eW), (dx, eL + eu)), (bt, bs, bx)))
    return out


def cl_judge(cls, got, ref, bnd):
    """one output array against its exact (I, e): exact class equal, generic within the bound
    (an entry whose bound is zero -- a row block past D -- must be an exact zero)"""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    I, e = ref
    I, bnd = np.asarray(I, dtype=object).reshape(-1), np.asarray(bnd, dtype=np.float64).reshape(-1)
    if not np.all(np.isfinite(got)):
        return False, float("inf")
    if cls == "exact":
        ok = rc.same(rc.ints(got[None]), (I, e))
        return ok, 0.0 if ok else float("inf")
    z = bnd == 0.0
    if np.any(got[z] != 0.0) or np.any(I[z] != 0):
        return False, float("inf")
    if np.all(z):
        return True, 0.0
    fig = rc.ratio(got[None, ~z], (I[~z], e), bnd[~z])
    return fig <= 1.0, fig


def ints_to_limbs(ref, words):
    """(I, e) -> limbs (words, n): limb q the nearest double of what the limbs before it leave
    (what a correct kernel would return where the value fits the width; reduce_cases.to_limbs
    without mpmath, for arenas of 10^5 entries)"""
    import math
    I, e = ref
    I = np.asarray(I, dtype=object).reshape(-1)
    out = np.zeros((words, I.size))
    for i, v in enumerate(I):
        r = int(v)
        for q in range(words):
            if r == 0:
                break
            sh = max(0, r.bit_length() - 900)
            top = r >> sh
            if sh and r & ((1 << sh) - 1):
                top |= 1                                         # (sticky: the rounding of top is r's)
            h = float(top)
            out[q, i] = math.ldexp(h, sh + e)
            r -= int(h) << sh
    return out
