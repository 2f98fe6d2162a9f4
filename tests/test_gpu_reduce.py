"""GPU tests of the reductions and slab sums on their own (clrsdp_reduce / clrsdp_slab_sum,
include/clrsdp.h): flat_reduce with its fold and with its tree, vec_reduce, the folds inside
scalar_kernel (fold_all_f64 at fp64, fold_wave at multi-word), ordered_reduce, slab_sum4 and
slab_qsolve, at words 1, 2 and 4 and at the smallest sizes that reach every thread-count and chunk
edge.  Operand classes, references, the bound and the checks are those of tests/reduce_cases.py:
the exact class must be the exact sum as a value, the generic (cancelling) class within
(n + 2) u sum |a b|, an extreme -- or a NaN -- must be found at every structurally distinct
position, with runner-ups that differ in the last limb only.  Every NaN that pads a gap or a guard
zone must stay unread and unwritten.  Each test prints its largest error / bound.

tests/test_reduce_host.py shows without a GPU that these checks reject a subtly wrong kernel."""
import numpy as np
import pytest

import reduce_cases as rc

pytestmark = pytest.mark.gpu

WORDS = list(rc.WORDS)
_cache = {}


def _pair(kind, n, words, parts=1):
    """(a, b, da, db) of a class at length n, computed once and left unchanged"""
    key = (kind, n, words, parts)
    if key not in _cache:
        if kind == "exact":
            v = rc.exact_pair(n, words, 21, parts) + rc.exact_pair(n, words, 23, parts)
        else:
            v = rc.generic_pair(n, words, 21) + tuple(0.25 * x for x in rc.generic_pair(n, words, 23))
        for x in v:
            x.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _ref(kind, n, words, op, parts=1):
    key = ("ref", kind, n, words, op, parts)
    if key not in _cache:
        a, b, da, db = _pair(kind, n, words, parts)
        if op == "dot":
            _cache[key] = (rc.dot_ints(a, b), rc.dot_bound(words, a, b))
        else:
            _cache[key] = (rc.dot_ints(a, b, da, db), rc.dot_bound(words, a, b, da, db))
    return _cache[key]


def _vec_points(words):
    nt, u = rc.NT[words], rc.U[words]
    pts = [1, nt - 1, nt, nt + 1, u * nt - 1, u * nt, u * nt + 1]
    pts += [u * nt + k * nt + 1 for k in range(u - 1)]           # each arm of the remainder
    return sorted(set(pts + [2 * u * nt + 1]))


def _extremes(pk, run, n, words, ops, chunk=None, seed=31):
    """an extreme and a NaN at every distinct position, for each op: bitwise the extreme, NaN"""
    for op in ops:
        for pos in rc.positions(n, words, chunk):
            v, want = rc.extreme_vector(n, words, seed, pos, op)
            got = run(v, op)
            assert rc.bitwise(got, want), (op, n, pos, got, want)
            v, _ = rc.extreme_vector(n, words, seed, pos, op, nan=True)
            got = run(v, op)
            assert rc.is_nan(got), f"{op} n={n}: the NaN at {pos} was dropped, result {got}"


# ---- vec_reduce ---------------------------------------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
def test_vec_dot(pk, words):
    worst = 0.0
    for n in _vec_points(words):
        for kind in ("exact", "generic"):
            a, b, _, _ = _pair(kind, n, words)
            got = pk.reduce("vec", a, b, op="dot", precision_words=words)
            ref, bnd = _ref(kind, n, words, "dot")
            ok, fig = rc.judge(kind, got, ref, bnd)
            assert ok, f"vec_reduce dot {kind} words={words} n={n}: {got} (error / bound {fig:.3e})"
            worst = max(worst, fig)
    print(f"REDUCE vec dot words={words}: error / bound = {worst:.3e}")


@pytest.mark.parametrize("words", WORDS)
def test_vec_maxabs(pk, words):
    for n in _vec_points(words):
        _extremes(pk, lambda v, op: pk.reduce("vec", v, op="maxabs", precision_words=words), n, words,
                  ("maxabs",))


# ---- flat_reduce with its fold and with its tree ------------------------------------------------
FLAT_N = [1, 255, 256, 257, 300, 65535, 65536, 65537, 4 * 65536 - 1, 4 * 65536 + 1]


@pytest.mark.parametrize("n", FLAT_N)
@pytest.mark.parametrize("words", WORDS)
def test_flat_sums(pk, words, n):
    """dot and dot-of-sums through flat_reduce + fold and flat_reduce + tree: both against the
    exact reference; on the exact class bitwise equal to each other, the partials summing to the
    reference, and a workgroup that owns nothing leaving an exact zero"""
    chunk = rc.flat_chunk(n)
    worst = 0.0
    for op in ("dot", "dotsum"):
        for kind in ("exact", "generic"):
            a, b, da, db = _pair(kind, n, words, parts=2)
            extra = dict(da=da, db=db) if op == "dotsum" else {}
            res = {}
            for k in ("flat_fold", "flat_tree"):
                got, part = pk.reduce(k, a, b, op=op, precision_words=words, return_partials=True, **extra)
                ref, bnd = _ref(kind, n, words, op, parts=2)
                ok, fig = rc.judge(kind, got, ref, bnd)
                assert ok, f"{k} {op} {kind} words={words} n={n}: {got} (error / bound {fig:.3e})"
                worst = max(worst, fig)
                res[k] = (got, part)
                owned = -(-n // chunk)
                assert np.all(part[:, owned:] == 0.0), f"{k} {op} n={n}: an empty workgroup's partial"
                if kind == "exact":
                    I, e = rc.ints(part)
                    assert rc.same((np.array([I.sum()], dtype=object), e), ref), f"{k} {op} n={n}: partials"
            assert rc.bitwise(res["flat_fold"][1], res["flat_tree"][1]), (op, kind, n)
            if kind == "exact":
                assert rc.bitwise(res["flat_fold"][0], res["flat_tree"][0]), (op, n)
    print(f"REDUCE flat words={words} n={n}: error / bound = {worst:.3e}")


@pytest.mark.parametrize("n", FLAT_N)
@pytest.mark.parametrize("words", WORDS)
def test_flat_maxabs(pk, words, n):
    for k in ("flat_fold", "flat_tree"):
        _extremes(pk, lambda v, op: pk.reduce(k, v, op="maxabs", precision_words=words), n, words,
                  ("maxabs",), chunk=rc.flat_chunk(n))


# ---- the folds of scalar_kernel -----------------------------------------------------------------
FOLD_CNT = [1, 2, 63, 64, 65, 255, 256, 257, 513]


def _run_folds(pk, words, items, per_call=12):
    """items = [(values (words, cnt), stride, op)]: every fold in an arena of its own stretch,
    the gaps between the strided values and between the folds NaN; per_call folds per call"""
    out = []
    for i0 in range(0, len(items), per_call):
        batch = items[i0:i0 + per_call]
        off, folds = 1, []
        for v, st, op in batch:
            folds.append((v.shape[1], st, off, op))
            off += (v.shape[1] - 1) * st + 2
        arena = np.full((words, off), np.nan)
        for (v, st, op), (cnt, _, o, _) in zip(batch, folds):
            arena[:, o:o + (cnt - 1) * st + 1:st] = v
        res = pk.reduce("fold", arena, folds=folds, precision_words=words)
        out += [res[:, q] for q in range(len(batch))]
    return out


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("words", WORDS)
def test_fold_sums(pk, words, stride):
    """each cnt on its own launch and all of them twelve to a call; fp64 also bitwise the
    documented order (lane l takes l, l + 64, ..., then the xor butterfly 32 .. 1)"""
    items, refs = [], []
    for cnt in FOLD_CNT:
        for kind in ("exact", "generic"):
            v = rc.exact_vector(cnt, words, 41) if kind == "exact" else rc.generic_vector(cnt, words, 41)
            items.append((v, stride, "sum"))
            refs.append((kind, cnt, rc.sum_ints(v), rc.sum_bound(words, v)))
    worst = 0.0
    for per_call in (1, 12):
        got = _run_folds(pk, words, items, per_call)
        for g, (v, _, _), (kind, cnt, ref, bnd) in zip(got, items, refs):
            ok, fig = rc.judge(kind, g, ref, bnd)
            assert ok, f"fold sum {kind} words={words} cnt={cnt} stride={stride}: {g} ({fig:.3e})"
            worst = max(worst, fig)
            if words == 1:
                assert g[0] == rc.fold_sum_f64(v[0]), f"fold order, cnt={cnt} stride={stride} {kind}"
    print(f"REDUCE fold sum words={words} stride={stride}: error / bound = {worst:.3e}")


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("words", WORDS)
def test_fold_extremes(pk, words, stride):
    items, want = [], []
    for cnt in FOLD_CNT:
        for op in ("max", "min", "maxabs"):
            for pos in rc.positions(cnt, words):
                for nan in (False, True):
                    v, w = rc.extreme_vector(cnt, words, 43, pos, op, nan=nan)
                    items.append((v, stride, op))
                    want.append((cnt, op, pos, nan, w))
    got = _run_folds(pk, words, items)
    for g, (cnt, op, pos, nan, w) in zip(got, want):
        if nan:
            assert rc.is_nan(g), f"fold {op} cnt={cnt} stride={stride}: the NaN at {pos} was dropped: {g}"
        else:
            assert rc.bitwise(g, w), (op, cnt, stride, pos, g, w)


@pytest.mark.parametrize("words", WORDS)
def test_six_and_seven_folds_in_one_call(pk, words):
    """six folds of unlike cnt and op share one launch (cnt 1 beside cnt 513); a seventh forces
    the second launch; every slot must be its own fold's"""
    spec = [(1, "sum"), (513, "sum"), (65, "maxabs"), (2, "min"), (257, "max"), (64, "sum"), (63, "min")]
    for count in (6, 7):
        for stride in (1, 3):
            items, want = [], []
            for q, (cnt, op) in enumerate(spec[:count]):
                if op == "sum":
                    v = rc.exact_vector(cnt, words, 50 + q)
                    want.append(rc.sum_ints(v))
                else:
                    v, w = rc.extreme_vector(cnt, words, 50 + q, cnt - 1, op)
                    want.append(w)
                items.append((v, stride, op))
            got = _run_folds(pk, words, items, per_call=count)
            for q, (g, w) in enumerate(zip(got, want)):
                if isinstance(w, tuple):
                    assert rc.value_equal(g, w), (count, stride, q, g)
                    if words == 1:
                        assert g[0] == rc.fold_sum_f64(items[q][0][0])
                else:
                    assert rc.bitwise(g, w), (count, stride, q, g, w)


# ---- ordered_reduce -----------------------------------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
def test_ordered_min(pk, words):
    for cnt in (1, 2, 7):
        for stride in (1, 3):
            for pos in range(cnt):
                for nan in (False, True):
                    v, w = rc.extreme_vector(cnt, words, 61, pos, "min", nan=nan)
                    arena = np.full((words, (cnt - 1) * stride + 1), np.nan)
                    arena[:, ::stride] = v
                    got = pk.reduce("ordered", arena, op="min", stride=stride, n=cnt, precision_words=words)
                    if nan:
                        assert rc.is_nan(got), f"ordered min cnt={cnt}: the NaN at {pos} was dropped: {got}"
                    else:
                        assert rc.bitwise(got, w), (cnt, stride, pos, got, w)


# ---- slab_sum4 and slab_qsolve ------------------------------------------------------------------
SLAB_CNT = [1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 65]
GUARD = 3


def _slabs(kind, cnt, n, words, pad=3, seed=71):
    """(slabs (words, cnt, n + pad) with NaN padding, the values (words, cnt, n))"""
    key = ("slab", kind, cnt, n, words, seed)
    if key not in _cache:
        flat = (rc.exact_vector(cnt * n, words, seed, m=2 ** 18 - 1) if kind == "exact"
                else rc.generic_vector(cnt * n, words, seed))
        val = flat.reshape(words, cnt, n)
        sl = np.full((words, cnt, n + pad), np.nan)
        sl[:, :, :n] = val
        base = (rc.exact_vector(n, words, seed + 1, m=2 ** 18 - 1) if kind == "exact"
                else rc.generic_vector(n, words, seed + 1, cancel=False))
        _cache[key] = (sl, val, base)
    return _cache[key]


def _slab_ref(words, val, base, cbase, csum):
    S = rc.colsum_ints(val)
    absum = np.sum(np.abs(val[0]), axis=0)
    if base is None:
        return S, rc.SLACK * (val.shape[1] + 2) * rc.EPS[words] * absum
    ref = rc.add(rc.scale(rc.ints(base), cbase), rc.scale(S, csum))
    return ref, rc.SLACK * (val.shape[1] + 3) * rc.EPS[words] * (abs(cbase) * np.abs(base[0]) + abs(csum) * absum)


def _guards_intact(out, n):
    g = np.full(out[:, :GUARD].shape, rc.NAN_PAYLOAD)
    return rc.bitwise(out[:, :GUARD], g) and rc.bitwise(out[:, GUARD + n:], g)


@pytest.mark.parametrize("cnt", SLAB_CNT)
@pytest.mark.parametrize("words", WORDS)
def test_slab_sum4(pk, words, cnt):
    """empty quarter-chunks (cnt < 4), the 8-unroll inside a chunk (cnt 32, 33, 65), elements on
    either side of the 64-wide workgroup; stride > n with NaN in the padding; without base and
    with out2, with base; NaN guard zones round out and out2"""
    worst = 0.0
    for n in (1, 63, 64, 65, 129):
        for kind in ("exact", "generic"):
            sl, val, base = _slabs(kind, cnt, n, words)
            out, out2 = pk.slab_sum(sl, n, out2=True, guard=GUARD, precision_words=words)
            assert _guards_intact(out, n) and _guards_intact(out2, n), (kind, cnt, n)
            got = out[:, GUARD:GUARD + n]
            assert rc.bitwise(got, out2[:, GUARD:GUARD + n])
            ref, bnd = _slab_ref(words, val, None, 0.0, 1.0)
            ok, fig = rc.judge(kind, got, ref, bnd)
            assert ok, f"slab_sum4 {kind} words={words} cnt={cnt} n={n}: error / bound {fig:.3e}"
            worst = max(worst, fig)
            out = pk.slab_sum(sl, n, base=base, cbase=1.0, csum=-1.0, guard=GUARD, precision_words=words)
            assert _guards_intact(out, n), (kind, cnt, n)
            ref, bnd = _slab_ref(words, val, base, 1.0, -1.0)
            ok, fig = rc.judge(kind, out[:, GUARD:GUARD + n], ref, bnd)
            assert ok, f"slab_sum4 base {kind} words={words} cnt={cnt} n={n}: error / bound {fig:.3e}"
            worst = max(worst, fig)
    print(f"REDUCE slab_sum4 words={words} cnt={cnt}: error / bound = {worst:.3e}")


def _padded(Q, pad=3):
    """Q with `pad` NaN rows below it (ldq = n + pad)"""
    return np.vstack([Q, np.full((pad, Q.shape[1]), np.nan)])


@pytest.mark.parametrize("cnt", SLAB_CNT)
def test_slab_qsolve(pk, cnt):
    """Q = I: bitwise slab_sum4's r; an integer Q on the exact class: the exact product; generic
    data: within the bound of r and of Q r composed,
      |Q| bound(r) + (n + 2) u |Q| (|r| + bound(r)).
    ldq = n + 3 with NaN in the padding rows, which are never read"""
    worst = 0.0
    u = rc.EPS[1]
    for n in (1, 2, 63, 64, 65, 127, 128):
        for kind in ("exact", "generic"):
            sl, val, base = _slabs(kind, cnt, n, 1)
            r4 = pk.slab_sum(sl, n, base=base, cbase=1.0, csum=-1.0)
            out = pk.slab_sum(sl, n, base=base, cbase=1.0, csum=-1.0, Q=_padded(np.eye(n)), guard=GUARD)
            assert _guards_intact(out, n), (kind, cnt, n)
            assert rc.bitwise(out[:, GUARD:GUARD + n], r4), f"slab_qsolve Q = I {kind} cnt={cnt} n={n}"
            rg = rc.rng(73, cnt, n)
            if kind == "exact":
                Q = rg.integers(-8, 9, size=(n, n)).astype(np.float64)
            else:
                Q = rg.uniform(-1.0, 1.0, size=(n, n))
            out = pk.slab_sum(sl, n, base=base, cbase=1.0, csum=-1.0, Q=_padded(Q), guard=GUARD)
            assert _guards_intact(out, n), (kind, cnt, n)
            r, br = _slab_ref(1, val, base, 1.0, -1.0)
            ref = rc.matvec_ints(Q, r)
            absr = np.abs(base[0]) + np.sum(np.abs(val[0]), axis=0)          # >= |r|
            bnd = np.abs(Q) @ br + rc.SLACK * (n + 2) * u * (np.abs(Q) @ (absr + br))
            ok, fig = rc.judge(kind, out[:, GUARD:GUARD + n], ref, bnd)
            assert ok, f"slab_qsolve {kind} cnt={cnt} n={n}: error / bound {fig:.3e}"
            worst = max(worst, fig)
    print(f"REDUCE slab_qsolve cnt={cnt}: error / bound = {worst:.3e}")
