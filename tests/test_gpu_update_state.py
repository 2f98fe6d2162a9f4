"""GPU tests of update_state on its own (clrsdp_update_state, include/clrsdp.h): the update of
X, Y, x, y under the status-word guard, the three rows of per-workgroup partials, and the fused
path that forms lambda_min and the step lengths itself, at words 1, 2 and 4.

Sizes: nel on either side of a workgroup's 4 x 256 prefetch (256 workgroups: 256 * 1024 - 1,
256 * 1024, 256 * 1024 + 1), below one element per workgroup (1), chunks of 2 with workgroups that
own nothing (257, 300); nx from 0 (a rank without clusters) to 4097, ny from 1 to 300.

Checks (operand classes and exact arithmetic of tests/reduce_cases.py):
  update    exact class (integers, alpha in {1, 1/2, 1/4}, steps multiples of 4): the new state is
            the exact one as a value; generic class: within 2 u (|v| + |alpha dv|) per element.
            Every element's leading limb is compared; the exact comparison of all limbs covers the
            whole array up to 8192 elements and beyond that every chunk's and the prefetch's edges
            plus a random sample.
  partials  row 0 is bitwise clrsdp_reduce's flat_reduce partials of the returned X and Y (the
            kernel's claim); the sums of rows 1 and 2 are <c, x_new> and <b, y_new>.
  guard     one status word set, at each position that another thread reads: nothing is written,
            the partials are those of the unchanged state.
  fused     the minima are exact at every position, alpha is the reference formula's at the
            precision of the operators, pd_feas equalises the steps, and the slot path given the
            same alpha leaves bitwise the same state."""
import numpy as np
import pytest

import reduce_cases as rc

pytestmark = pytest.mark.gpu

WORDS = list(rc.WORDS)
G = rc.RED_G
# relative precision of one division of the multi-word operators (tests/test_host.py)
DIV_TOL = {1: 2.0 ** -53, 2: 2.0 ** -100, 4: 2.0 ** -203}
_cache = {}


# ---- states (no GPU: tests/test_reduce_host.py uses them too) -----------------------------------
def exact_state(nel, nx, ny, words, seed):
    """integers with n (2 m)^2 < 2^50 for every sum of the new state; the steps are multiples of 4
    (so alpha = 1/4 keeps integers) of at most half the magnitude of the state; one factor of
    every product has a single limb"""
    def pair(n, s, trailing):
        m = rc.amax(max(n, 1), 2)
        m -= m % 8
        m = max(m, 8)
        v = rc.exact_vector(n, words, s, m=m, trailing=trailing)
        dv = rc.exact_vector(n, words, s + 1, m=max(4, m // 2), trailing=trailing, mult=4.0)
        return v, dv
    X, dX = pair(nel, seed, True)
    Y, dY = pair(nel, seed + 2, False)
    x, dx = pair(nx, seed + 4, True)
    y, dy = pair(ny, seed + 6, True)
    c = rc.exact_vector(nx, words, seed + 8, m=rc.amax(max(nx, 1), 2), trailing=False)
    b = rc.exact_vector(ny, words, seed + 9, m=rc.amax(max(ny, 1), 2), trailing=False)
    return dict(X=X, dX=dX, Y=Y, dY=dY, x=x, dx=dx, c=c, y=y, dy=dy, b=b)


def generic_state(nel, nx, ny, words, seed):
    g = lambda n, s, f=1.0: rc.generic_vector(n, words, s, cancel=False) * f
    return dict(X=g(nel, seed), dX=g(nel, seed + 1, 0.5), Y=g(nel, seed + 2), dY=g(nel, seed + 3, 0.5),
                x=g(nx, seed + 4), dx=g(nx, seed + 5, 0.5), c=g(nx, seed + 6), y=g(ny, seed + 7),
                dy=g(ny, seed + 8, 0.5), b=g(ny, seed + 9))


def updated(st, ap, ad):
    """limb by limb v + alpha dv for a power of two alpha on the exact class: every limb exact
    (the limbs of the result need not be the device's; the values are)"""
    return dict(X=st["X"] + ap * st["dX"], Y=st["Y"] + ad * st["dY"], x=st["x"] + ap * st["dx"],
                y=st["y"] + ad * st["dy"])


def _state(kind, nel, nx, ny, words):
    key = (kind, nel, nx, ny, words)
    if key not in _cache:
        st = (exact_state if kind == "exact" else generic_state)(nel, nx, ny, words, 81)
        for v in st.values():
            v.setflags(write=False)
        _cache[key] = st
    return _cache[key]


def _sample(n):
    """all of a short array; of a long one both ends, every flat chunk's first and last elements,
    the elements round the 4 x 256 prefetch of every chunk, and 2048 random ones"""
    if n <= 8192:
        return np.arange(n)
    chunk = rc.flat_chunk(n)
    lo = np.arange(G) * chunk
    idx = [np.arange(64), np.arange(n - 64, n), rc.rng(83, n).integers(0, n, 2048)]
    for d in (-1, 0, 1, 255, 256, 1023, 1024, 1025, chunk - 2, chunk - 1):
        idx.append(lo + d)
    idx = np.unique(np.concatenate(idx))
    return idx[(idx >= 0) & (idx < n)]


def _alpha_limbs(alpha, words):
    from clrsdp_amd.solver import limbs
    return np.array(limbs(alpha, words))


def _check_update(kind, words, got, v, dv, alpha, what):
    """got = v + alpha dv: the leading limb of every element, every limb of the sampled ones"""
    if v.shape[1] == 0:
        assert got.shape[1] == 0
        return 0.0
    al = _alpha_limbs(alpha, words)
    lead = v[0] + al[0] * dv[0]
    # exact class: the integer part, and where it cancels to zero the trailing part (below 2^-70)
    # moves up into the leading limb
    tol = 2.0 ** -70 if kind == "exact" else 4.0 * rc.EPS[1] * (np.abs(v[0]) + np.abs(dv[0]))
    assert np.all(np.abs(got[0] - lead) <= tol), f"{what}: leading limbs"
    idx = _sample(v.shape[1])
    ref = rc.add(rc.ints(v[:, idx]), (rc.ints(dv[:, idx])[0] * rc.ints(al)[0][0],
                                      rc.ints(dv[:, idx])[1] + rc.ints(al)[1]))
    bnd = 2.0 * rc.EPS[words] * (np.abs(v[0, idx]) + abs(al[0]) * np.abs(dv[0, idx]))
    ok, fig = rc.judge(kind, got[:, idx], ref, bnd)
    assert ok, f"{what} {kind} words={words}: error / bound {fig:.3e}"
    return fig


def _check_partials(pk, kind, words, res, c, b, what):
    """row 0 against flat_reduce of the returned X, Y; rows 1 and 2 against <c, x> and <b, y> of
    the returned x, y"""
    _, part = pk.reduce("flat_fold", res["X"], res["Y"], op="dot", precision_words=words,
                        return_partials=True)
    assert rc.bitwise(res["part"][:, 0], part), f"{what}: the <X,Y> partials are not flat_reduce's"
    worst = 0.0
    for row, (u, v) in ((1, (c, res["x"])), (2, (b, res["y"]))):
        p = res["part"][:, row]
        assert np.all(np.isfinite(p)), f"{what}: partials row {row}"
        if u.shape[1] == 0:
            assert np.all(p == 0.0), f"{what}: partials of an empty vector"
            continue
        I, e = rc.ints(p)
        tot = (np.array([I.sum()], dtype=object), e)
        ref = rc.dot_ints(u, v)
        if kind == "exact":
            assert rc.same(tot, ref), f"{what}: the sum of partials row {row}"
        else:
            r = rc.ratio(rc.to_limbs(tot, 4)[:, 0], ref, rc.dot_bound(words, u, v))
            assert r <= 1.0, f"{what}: partials row {row}, error / bound {r:.3e}"
            worst = max(worst, r)
    return worst


SIZES = [(1, 0, 1), (257, 1, 64), (300, 255, 300), (256 * 1024 - 1, 257, 1), (256 * 1024, 4097, 64),
         (256 * 1024 + 1, 0, 300), (300, 4097, 1)]
ALPHAS = [(1.0, 0.5), (0.5, 0.25), (0.25, 1.0)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "nel%d-nx%d-ny%d" % s)
@pytest.mark.parametrize("words", WORDS)
def test_update_and_partials(pk, words, size):
    nel, nx, ny = size
    worst = 0.0
    for kind in ("exact", "generic"):
        st = _state(kind, nel, nx, ny, words)
        ap, ad = ALPHAS[SIZES.index(size) % 3] if kind == "exact" else ("0.7316", "0.4153")
        res = pk.update_state(**st, info=np.zeros(5, dtype=np.int32),
                              alpha=(_alpha_limbs(ap, words), _alpha_limbs(ad, words)), precision_words=words)
        what = f"update_state nel={nel} nx={nx} ny={ny}"
        for k, dk, al in (("X", "dX", ap), ("Y", "dY", ad), ("x", "dx", ap), ("y", "dy", ad)):
            worst = max(worst, _check_update(kind, words, res[k], st[k], st[dk], al, what + " " + k))
        worst = max(worst, _check_partials(pk, kind, words, res, st["c"], st["b"], what))
    print(f"UPDATE words={words} nel={nel} nx={nx} ny={ny}: error / bound = {worst:.3e}")


NINFO = 300


@pytest.mark.parametrize("words", WORDS)
def test_guard_on_the_slot_path(pk, words):
    """the status words are read by all 256 threads, stride 256"""
    st = _state("exact", 300, 255, 64, words)
    al = (_alpha_limbs(0.5, words), _alpha_limbs(0.25, words))
    for pos in (0, 63, 64, 255, 256, NINFO - 1):
        info = np.zeros(NINFO, dtype=np.int32)
        info[pos] = 1 + pos
        res = pk.update_state(**st, info=info, alpha=al, precision_words=words)
        for k in ("X", "Y", "x", "y"):
            assert rc.bitwise(res[k], st[k]), f"status word {pos} set, but {k} was written"
        _check_partials(pk, "exact", words, res, st["c"], st["b"], f"guard at {pos}")


def _eigs(nblk, words, pos, small):
    """nblk eigenvalues with the minimum -E at pos and runner-ups that differ in the last limb;
    `small`: scaled by 1/8, so that the minimum stays above -gamma"""
    v, want = rc.extreme_vector(nblk, words, 91, pos, "min")
    return (v * 0.125, want * 0.125) if small else (v, want)


def _alpha_ref(minv, gamma, words):
    import mpmath
    with mpmath.workprec(400):
        m = mpmath.fsum([mpmath.mpf(float(t)) for t in minv])
        g = mpmath.fsum([mpmath.mpf(float(t)) for t in gamma])
        return mpmath.mpf(1) if m > -g else -g / m


def _close(got, ref, words):
    import mpmath
    with mpmath.workprec(400):
        g = mpmath.fsum([mpmath.mpf(float(t)) for t in got])
        return abs(g - ref) <= DIV_TOL[words] * abs(ref)


@pytest.mark.parametrize("words", WORDS)
def test_guard_on_the_fused_path(pk, words):
    """there wave 0 forms alpha and threads 64 .. 255 read the status words, stride 192"""
    st = _state("exact", 300, 255, 64, words)
    gamma = _alpha_limbs("0.7", words)
    ex, _ = _eigs(65, words, 64, False)
    ey, _ = _eigs(65, words, 0, True)
    for pos in (0, 191, 192, NINFO - 1):
        info = np.zeros(NINFO, dtype=np.int32)
        info[pos] = -1
        res = pk.update_state(**st, info=info, eig=(ex, ey), gamma=gamma, precision_words=words)
        for k in ("X", "Y", "x", "y"):
            assert rc.bitwise(res[k], st[k]), f"status word {pos} set, but {k} was written"
        _check_partials(pk, "exact", words, res, st["c"], st["b"], f"fused guard at {pos}")


@pytest.mark.parametrize("nblk", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("words", WORDS)
def test_fused_minima_and_step_lengths(pk, words, nblk):
    import mpmath
    st = _state("generic", 300, 5, 7, words)
    gamma = _alpha_limbs("0.7", words)
    info = np.zeros(4, dtype=np.int32)
    for pos in range(nblk):      # the minimum, and a NaN, at every position (min_fold64)
        ex, mx = _eigs(nblk, words, pos, False)
        ey, my = _eigs(nblk, words, nblk - 1 - pos, True)
        step = pk.update_state(**st, info=info, eig=(ex, ey), gamma=gamma, precision_words=words)["step"]
        assert rc.bitwise(step[:, 0], mx) and rc.bitwise(step[:, 1], my), f"minima, nblk={nblk} pos={pos}"
        ex[0, pos] = np.nan
        step = pk.update_state(**st, info=info, eig=(ex, ey), gamma=gamma, precision_words=words)["step"]
        assert rc.is_nan(step[:, 0]) and rc.bitwise(step[:, 1], my), \
            f"nblk={nblk}: the NaN eigenvalue at {pos} was dropped: {step[:, 0]}"
    for pos in sorted({0, nblk - 1, nblk // 2} | {p for p in (63, 64, 65) if p < nblk}):
        # (X below -gamma, Y above), (X above, Y below), both below
        for sx, sy in ((False, True), (True, False), (False, False)):
            ex, mx = _eigs(nblk, words, pos, sx)
            ey, my = _eigs(nblk, words, nblk - 1 - pos, sy)
            ey, my = ey * 0.5, my * 0.5
            for pd in (False, True):
                res = pk.update_state(**st, info=info, eig=(ex, ey), gamma=gamma, pd_feas=pd,
                                      precision_words=words)
                step = res["step"]
                what = f"fused nblk={nblk} pos={pos} small=({sx},{sy}) pd_feas={pd} words={words}"
                assert rc.bitwise(step[:, 0], mx) and rc.bitwise(step[:, 1], my), what + ": minima"
                ap, ad = _alpha_ref(mx, gamma, words), _alpha_ref(my, gamma, words)
                with mpmath.workprec(400):
                    assert (ap == 1) == sx and (ad == 1) == sy, what      # min > -gamma, or not
                    if pd:
                        ap = ad = min(ap, ad)
                assert _close(step[:, 2], ap, words) and _close(step[:, 3], ad, words), what + ": alpha"
                if pd:
                    assert rc.bitwise(step[:, 2], step[:, 3]), what
                # the slot path with this alpha: the same state and partials, bitwise
                slot = pk.update_state(**st, info=info, alpha=(step[:, 2], step[:, 3]), precision_words=words)
                for k in ("X", "Y", "x", "y", "part"):
                    assert rc.bitwise(res[k], slot[k]), what + f": {k} differs from the slot path's"
