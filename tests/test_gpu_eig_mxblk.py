"""lambda_min of multi-word blocks past the LDS kernels by the mxblk route (CLRSDP_EIG_MX_BLK=1;
mxblk_* in csrc/kernels_dense.h): the fp64 eigblk_* chain on the leading limbs, an fp64 Cholesky
factor of A_h - mu I as the correction operator, refinement steps at the word's width accepted by
Temple's bound, and the route the switch replaced on the blocks it flags.

Tolerance: that of test_gpu_eig_blk.py, EIG_TOL[words] max(1, n/64) of the block's spectral
radius.  Blocks and batch layout: test_gpu_eigmin_sizes.py (its helpers as they are, the
known-spectrum blocks built once for all three files).  Every test prints its worst
error / tolerance, the routes (clrsdp_eigmin_routes: 0 certified by the refinement, 1 flagged and
computed by the fallback launch) and, from the CLRSDP_EIGMX_STATS=1 line of the call, the most
refinement steps a certified block took.

The random symmetric blocks have binary64 entries, so they are exact at every width; their
reference is a certificate, not an eigen-solve: numpy's eigenpair refined at 320 bits (mpmath
matrix-vector products, the fp64 inverse of A - mu I as the correction), then Temple's bound
rho - eta / (lam2 - rho) <= lambda_min <= rho with lam2 numpy's second eigenvalue less 1e-9 of the
radius (numpy's own error is ~1e-14 of it); the width eta / (lam2 - rho) is asserted below 1e-70
of the radius, twenty digits inside the quad-double tolerance.

Routes asserted: the tiny-minimum block, the random block and the spread spectrum with gap 2^-10
are certified (route 0: a run that passes only through the fallback fails); the triple minimum,
c I, the spread spectrum with gap 2^-60 and the riders with n < 3 are flagged (route 1).
Nothing is asserted for the decoupled and 2 x 2 tridiagonals.

Measured on an MI355X, worst error / tolerance (at the flagged triple-minimum block or a rider in
every batch, i.e. the fallback's own error): dispatch ranges dd 97 3.5e-4, 129 2.2e-4, 160
2.3e-4; qd 67 2.5e-14, 100 1.4e-14, 130 6.1e-15.  Scaled (the same figure at 2^120, 2^-120, 2^600
and 2^-600, at the certified tiny-minimum block): dd 128 4.0e-6, qd 80 1.3e-16.  Hadamard: dd 1024
3.9e-6, qd 512 4.0e-16, both certified.  Most refinement steps of a certified block: 1 at
double-double, 2 at quad-double, in every test.  Routes beyond the asserted ones: decoupled
certified at 97, 129 (dd) and 67 (qd), flagged at 160, 100, 130 and 128 / 80; 2 x 2 flagged
everywhere; the riders of n = 3, 17, 64 (gap 2^-60) flagged.  STEP stage, route against unset:
dd delta = 100 lambda 1.4e-4 of its bound (Y; X is flagged and bitwise equal), qd delta = 80
1.6e-14.
"""
import re

import mpmath
import numpy as np
import pytest

import test_gpu_eig_blk as eb
import test_gpu_eigmin_sizes as es
import test_gpu_step_large as tsl

pytestmark = pytest.mark.gpu

BATCHED, BLK, MXBLK = 4, 5, 6   # CLRSDP_EIG_K_* (include/clrsdp.h)
SWITCH = "CLRSDP_EIG_MX_BLK"
_RANDOM = {}


@pytest.fixture
def route(monkeypatch):
    monkeypatch.delenv("CLRSDP_EIG_MX", raising=False)
    monkeypatch.delenv("CLRSDP_EIG_BLK", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    monkeypatch.setenv("CLRSDP_EIGMX_STATS", "1")
    return monkeypatch


def _random_block(n, seed):
    """(block, lambda_min, spectral radius) of a dense random symmetric block with binary64
    entries; the reference by the certificate of the module docstring.  Built once."""
    key = (n, seed)
    if key in _RANDOM:
        return _RANDOM[key]
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A = (A + A.T) / 2
    w, V = np.linalg.eigh(A)
    rad = float(np.max(np.abs(w)))
    mu = w[0] - 1e-9 * rad
    Minv = np.linalg.inv(A - mu * np.eye(n))
    z = V[:, 0]
    with mpmath.workprec(320):
        Am = np.array([[mpmath.mpf(float(v)) for v in row] for row in A], dtype=object)
        x = np.array([mpmath.mpf(float(v)) for v in z], dtype=object)
        lam2 = mpmath.mpf(float(w[1])) - mpmath.mpf(1e-9) * rad
        for _ in range(8):
            y = Am.dot(x)
            den = mpmath.fsum(v * v for v in x)
            rho = mpmath.fsum(a * b for a, b in zip(x, y)) / den
            r = y - rho * x
            eta = mpmath.fsum(v * v for v in r) / den
            width = eta / (lam2 - rho)
            if width < mpmath.mpf(10) ** -75 * rad:
                break
            rf = np.array([float(v / mpmath.sqrt(eta)) for v in r])
            d = -Minv.dot(rf)
            d -= z * z.dot(d)
            x = x + np.array([mpmath.mpf(float(v)) for v in d], dtype=object) * mpmath.sqrt(eta)
        assert lam2 > rho and width < mpmath.mpf(10) ** -70 * rad, (n, seed, float(width))
        out = (A, rho, mpmath.mpf(rad))
    _RANDOM[key] = out
    return out


def _steps(capfd):
    """(flagged, blocks, most refinement steps) of the last call's CLRSDP_EIGMX_STATS line."""
    m = re.findall(r"eigmin_mxblk: (\d+) of (\d+) blocks flagged, most refinement steps of a certified block (\d+)",
                   capfd.readouterr().err)
    return tuple(int(v) for v in m[-1]) if m else None


def _check(pk, capfd, words, cases, label):
    """One clrsdp_eigmin_routes call over ``cases`` = [(name, kind, n, exponent, g)] (kind
    "random": g is the seed); every lambda_min to eb._tol(words, n) of the block's spectral
    radius.  Returns {name: route}."""
    refs = [_random_block(n, g) if kind == "random" else es._block(kind, n, g) for _, kind, n, _, g in cases]
    capfd.readouterr()
    got, routes = pk.eigmin([es._for_words(r[0], words, c[3]) for r, c in zip(refs, cases)],
                            precision_words=words, return_routes=True)
    stats = _steps(capfd)
    ratios, bad = [], []
    with mpmath.workprec(320):
        for (name, kind, n, ex, _), (_, lam, rad), gv in zip(cases, refs, got):
            gm = mpmath.mpf(gv)
            err = abs(mpmath.ldexp(gm, -ex) - lam) / rad
            ratio = float(err / eb._tol(words, n)) if mpmath.isfinite(err) else float("inf")
            ratios.append((ratio, name))
            if not ratio <= 1.0:
                bad.append((name, n, ex, str(gm), float(lam), ratio))
    w = max(ratios)
    by_name = {c[0]: int(r) for c, r in zip(cases, routes)}
    print(f"eigmin mxblk {label}: {len(cases)} blocks, worst error / tolerance {w[0]:.3g} at {w[1]}; "
          f"routes {by_name}; (flagged, blocks, most refinement steps) {stats}")
    assert not bad, f"(block, n, exponent, lambda_min, reference, error / tolerance): {bad}"
    assert stats is not None and stats[0] == sum(by_name.values()) and stats[1] == len(cases)
    return by_name


SIZES = [(2, 97), (2, 129), (2, 160), (4, 67), (4, 100), (4, 130)]


@pytest.mark.parametrize("words,nmax", SIZES)
def test_route_across_the_dispatch_ranges(pk, route, capfd, words, nmax):
    """The first size of each range, then ragged strips: one call per (words, nmax)."""
    assert pk.eigmin_kernel(nmax, words) == MXBLK
    cases = [(f"{k}{nmax}", k, nmax, 0, 60) for k in ("tiny", "spread", "triple", "cI", "decoupled", "2x2")]
    cases += [(f"random{nmax}", "random", nmax, 0, 7000 + nmax)]
    cases += [("rider1", "one", 1, 0, 60), ("rider2", "two", 2, 0, 60)]
    cases += [(f"rider{n}", "spread", n, 0, 60) for n in (3, 17, 64)]
    if (words, nmax) in ((2, 97), (4, 67)):
        cases += [(f"spread10_{nmax}", "spread", nmax, 0, 10)]
    r = _check(pk, capfd, words, cases, f"words={words} nmax={nmax}")
    certified = [f"tiny{nmax}", f"random{nmax}"] + ([f"spread10_{nmax}"] if len(cases) == 13 else [])
    flagged = [f"spread{nmax}", f"triple{nmax}", f"cI{nmax}", "rider1", "rider2"]
    assert all(r[k] == 0 for k in certified), {k: r[k] for k in certified}
    assert all(r[k] == 1 for k in flagged), {k: r[k] for k in flagged}


@pytest.mark.parametrize("ex", [120, -120, 600, -600])
@pytest.mark.parametrize("words,n", [(2, 128), (4, 80)])
def test_route_scaled_blocks(pk, route, capfd, words, n, ex):
    """The tiny-minimum block and the decoupled tridiagonal times 2^ex: the prepass divides the
    images and the matrix-vector products by the power of two of the block's largest
    leading-limb magnitude and rho is multiplied back."""
    assert pk.eigmin_kernel(n, words) == MXBLK
    cases = [(f"tiny{n}", "tiny", n, ex, 60), (f"decoupled{n}", "decoupled", n, ex, 60)]
    r = _check(pk, capfd, words, cases, f"words={words} n={n} scale=2^{ex}")
    assert r[f"tiny{n}"] == 0, r


@pytest.mark.parametrize("words,n,big", [(2, 110, 140), (4, 75, 90)])
def test_route_is_independent_of_the_batch(pk, route, words, n, big):
    """One block alone and as the third of a batch with a larger block: bitwise the same
    lambda_min and the same route (every sum is one thread's ascending sum or a fixed tree with
    one workgroup per block; the grids follow the batch's nmax)."""
    rng = np.random.default_rng(4300 + words)
    A, B, S = eb._sym(rng, n), eb._sym(rng, big), eb._sym(rng, 70)
    assert pk.eigmin_kernel(n, words) == MXBLK and pk.eigmin_kernel(big, words) == MXBLK
    alone, ra = pk.eigmin([A], precision_words=words, return_routes=True)
    batch, rb = pk.eigmin([B, S, A], precision_words=words, return_routes=True)
    ref = float(np.linalg.eigvalsh(A)[0])
    rad = float(np.max(np.abs(np.linalg.eigvalsh(A))))
    err = abs(float(alone[0]) - ref) / rad
    print(f"mxblk batch independence words={words} n={n}: lambda_min {float(alone[0]):.17g}, routes "
          f"{list(ra)} / {list(rb)}, against numpy / (n eps) {err / (n * 2.2e-16):.3g}")
    assert err <= n * 2.2e-16    # numpy's own backward error: a sanity check, not the precision test
    assert alone[0] == batch[2], (alone[0], batch[2])
    assert ra[0] == rb[2] == 0, (ra, rb)


@pytest.mark.parametrize("chain", [None, "1"])
@pytest.mark.parametrize("words,n", [(2, 97), (4, 67)])
def test_fallback_is_the_computation_of_the_replaced_route(pk, monkeypatch, words, n, chain):
    """The triple-minimum and c I blocks are flagged, and the block is only read before the
    fallback launch: lambda_min with the switch on is bitwise lambda_min with it unset, with
    CLRSDP_EIG_BLK unset (eigmin_batched) and =1 (the multi-word chain)."""
    monkeypatch.delenv("CLRSDP_EIG_MX", raising=False)
    if chain:
        monkeypatch.setenv("CLRSDP_EIG_BLK", chain)
    else:
        monkeypatch.delenv("CLRSDP_EIG_BLK", raising=False)
    blocks = [es._for_words(es._block(k, n, 60)[0], words) for k in ("triple", "cI")]
    monkeypatch.delenv(SWITCH, raising=False)
    assert pk.eigmin_kernel(n, words) == (BLK if chain else BATCHED)
    off = pk.eigmin(blocks, precision_words=words)
    monkeypatch.setenv(SWITCH, "1")
    assert pk.eigmin_kernel(n, words) == MXBLK
    on, routes = pk.eigmin(blocks, precision_words=words, return_routes=True)
    print(f"mxblk fallback words={words} n={n} chain={chain}: routes {list(routes)}, "
          f"lambda_min {[float(v) for v in on]}")
    assert list(routes) == [1, 1]
    assert all(a == b for a, b in zip(on, off)), (on, off)


def test_default_is_untouched(pk, monkeypatch):
    """With the switch unset and with 0, double-double 160 takes eigmin_batched, the results are
    bitwise equal and no route is reported."""
    monkeypatch.delenv("CLRSDP_EIG_BLK", raising=False)
    A = eb._sym(np.random.default_rng(161), 160)
    monkeypatch.delenv(SWITCH, raising=False)
    assert pk.eigmin_kernel(160, 2) == BATCHED
    unset, r0 = pk.eigmin([A], precision_words=2, return_routes=True)
    monkeypatch.setenv(SWITCH, "0")
    assert pk.eigmin_kernel(160, 2) == BATCHED
    zero, r1 = pk.eigmin([A], precision_words=2, return_routes=True)
    assert unset[0] == zero[0], (unset[0], zero[0])
    assert list(r0) == [-1] and list(r1) == [-1]
    assert pk.eigmin([A], precision_words=2)[0] == unset[0]


@pytest.mark.parametrize("words,n", [(2, 1024), (4, 512)])
def test_route_past_the_one_cu_launch_request(pk, route, capfd, words, n):
    """The Hadamard blocks of test_gpu_eig_blk.py (A_ij = f(i xor j), spectrum d exactly), where
    eigmin_batched's LDS request passes 64 KiB: the flagged blocks would go to the multi-word
    chain.  Accuracy only; the route is printed."""
    from clrsdp_amd import _lib
    from clrsdp_amd.instance import from_planes
    assert pk.eigmin_kernel(n, words) == MXBLK
    rng = np.random.default_rng(900 + words)
    d1 = rng.integers(-2**20 + 1, 2**20, n)
    d2 = rng.integers(-2**20 + 1, 2**20, n)
    f1 = eb._fwht(d1).astype(np.float64) / n
    f2 = np.ldexp(eb._fwht(d2).astype(np.float64) / n, -60)
    hi = f1 + f2
    lo = (f1 - (hi - (hi - f1))) + (f2 - (hi - f1))  # two-sum: hi + lo = f1 + f2 exactly
    idx = np.arange(n)[:, None] ^ np.arange(n)[None, :]
    planes = np.zeros((words, n * n))
    planes[0] = hi[idx].reshape(-1)
    planes[1] = lo[idx].reshape(-1)
    planes = planes.reshape(-1)
    out = np.zeros(words)
    nn = np.array([n], dtype=np.int64)
    rt = np.full(1, -2, dtype=np.int32)
    capfd.readouterr()
    _lib.check(_lib.lib().clrsdp_eigmin_routes(0, words, 1, nn.ctypes.data_as(_lib.P_i64),
                                               planes.ctypes.data_as(_lib.P_f64), out.ctypes.data_as(_lib.P_f64),
                                               rt.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))))
    stats = _steps(capfd)
    with mpmath.workprec(320):
        lam = [mpmath.mpf(int(a)) + mpmath.ldexp(mpmath.mpf(int(b)), -60) for a, b in zip(d1, d2)]
        ref, rad = min(lam), max(abs(v) for v in lam)
        got = from_planes(out, 1, words)[0]
        ratio = float(abs(got - ref) / rad / eb._tol(words, n))
    print(f"eigmin mxblk hadamard words={words} n={n}: worst error / tolerance {ratio:.3g}, route {int(rt[0])}, "
          f"(flagged, blocks, most refinement steps) {stats}")
    assert rt[0] in (0, 1)
    assert ratio <= 1.0, (float(got), float(ref), ratio)


# ---------------------------------------------------------------- through the solver

def _step_stage(pk, oracle, words, D, on, monkeypatch):
    """eb._step_stage with this file's switch on or unset when the handle is created
    (CLRSDP_EIG_BLK unset in both)."""
    if on:
        monkeypatch.setenv(SWITCH, "1")
    else:
        monkeypatch.delenv(SWITCH, raising=False)
    return eb._step_stage(pk, oracle, words, D, False, monkeypatch)


@pytest.mark.parametrize("words,D", [(2, 100), (4, 80)])
def test_step_stage_with_the_route(pk, oracle, monkeypatch, words, D):
    """STAGE_STEP with the route against the same stage with the switch unset, as
    test_gpu_eig_blk.test_step_stage_with_the_chain: each lambda slot to tol(n) rad, alpha to the
    same bound through alpha = min(1, -gamma / lambda) plus one rounding of the word."""
    monkeypatch.delenv("CLRSDP_EIG_MX", raising=False)
    bi, X, dX, Y, dY, off = _step_stage(pk, oracle, words, D, False, monkeypatch)
    assert pk.eigmin_kernel(D, words) == BATCHED
    _, _, _, _, _, on = _step_stage(pk, oracle, words, D, True, monkeypatch)
    assert pk.eigmin_kernel(D, words) == MXBLK
    tol = eb._tol(words, D)
    eps = {2: 2.5e-32, 4: 1.3e-63}[words]
    gamma = mpmath.mpf(tsl.GAMMA)
    worst = 0.0
    with mpmath.workprec(320):
        for M, dM, lk, ak in ((X, dX, "mineig_X", "alpha_p"), (Y, dY, "mineig_Y", "alpha_d")):
            rad = max(tsl._rad(np.array(M[j][l], dtype=object), np.array(dM[j][l], dtype=object))
                      for j in range(bi.J) for l in range(bi.L[j]))
            l1, l0 = mpmath.mpf(on[lk]), mpmath.mpf(off[lk])
            a1, a0 = mpmath.mpf(on[ak]), mpmath.mpf(off[ak])
            assert mpmath.isfinite(l1) and mpmath.isfinite(l0)
            lerr = float(abs(l1 - l0) / (tol * rad))
            abound = gamma * tol * rad / abs(l1 * l0) + 4 * eps * a0
            aerr = float(abs(a1 - a0) / abound)
            print(f"step mxblk words={words} D={D} {lk}: {float(l1):.17g} against {float(l0):.17g}, "
                  f"error / tolerance {lerr:.3g}; {ak} {float(a1):.17g} against {float(a0):.17g}, "
                  f"error / bound {aerr:.3g}")
            worst = max(worst, lerr, aerr)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("graph", [None, "1"])
def test_iterate_equals_the_stages_with_the_route(pk, oracle, route, graph):
    """Double-double, X/Y blocks of 100 and 12: clrsdp_iterate leaves bitwise the state and
    scalars of the ten stages run one by one, eager and with the loop body captured and
    replayed (CLRSDP_GRAPH_MW=1)."""
    from clrsdp_amd import _lib as L
    from clrsdp_amd import instance as inst
    if graph:
        route.setenv("CLRSDP_GRAPH_MW", graph)
    else:
        route.delenv("CLRSDP_GRAPH_MW", raising=False)
    assert pk.eigmin_kernel(100, 2) == MXBLK
    cons, b, bi, state = tsl._state(pk, oracle, 100)
    P = pk.make_params("0.3", "0.1", tsl.GAMMA, 0)
    got = []
    for whole in (False, True):
        dev = pk.DeviceSolver(cons, b, pk.get_block_info(cons), precision_words=2)
        try:
            dev.set_state(*state)
            if whole:
                dev.iterate(P, False)
            else:
                for s in range(L.STAGE_MU_R, L.STAGE_UPDATE + 1):
                    dev.run_stage(s, P, False)
            x, X, y, Y = dev.get_state(True)   # exact: the limb sums as mpmath numbers
            sc = dev.buffer(L.BUF_SCALARS, True)
            got.append((list(x), list(inst.blocks_to_flat(X)), list(y), list(inst.blocks_to_flat(Y)),
                        [sc[L.SC[k]] for k in ("mineig_X", "mineig_Y", "alpha_p", "alpha_d", "mu")]))
        finally:
            dev.close()
    for name, a, c in zip(("x", "X", "y", "Y", "scalars"), got[0], got[1]):
        assert len(a) == len(c) and all(u == v for u, v in zip(a, c)), name
    print(f"iterate against stages, mxblk route on, graph={graph}: mineig_X {float(got[1][4][0]):.17g}, "
          f"alpha_p {float(got[1][4][2]):.17g}")
