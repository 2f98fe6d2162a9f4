"""lambda_min by the eigblk_* chain (CLRSDP_EIG_BLK=1): the Householder tridiagonalisation of the
blocks past the LDS kernels across workgroups, one launch per column (eigblk_amax, eigblk_sym,
eigblk_col, eigblk_sturm in csrc/kernels_dense.h), in place of the one-CU eigmin_batched.

Tolerances, relative to the block's spectral radius: multi-word, EIG_TOL[words] max(1, n/64) with
EIG_TOL = {2: 1e-28, 4: 1e-50}; fp64, 1e-12 max(1, n/128) -- the "n eps ||T||" law of
test_gpu_eigmin_sizes.py, whose 1e-12 it is at n <= 128.  Every test prints its worst
error / tolerance.

Blocks and the batch layout of the dispatch-table and scale tests are those of
test_gpu_eigmin_sizes.py (its helpers are used as they are; the known-spectrum blocks are built
once for both files).  The chain rows: fp64 nmax >= 139, double-double >= 97, quad-double >= 67.
The sizes are the first of each range, then sizes with a ragged last strip at strips of 16, 32 and
64 rows and several strips; the trailing matrix shrinks by one row per launch, so every block passes
through every ragged remainder.  The c I, decoupled and 2 x 2 blocks are tridiagonal already
(beta = 0 in every column), and the riders of n = 1, 2, 3, 17, 64 leave the column launches at once.

Past the one-CU kernel's launch request (eigmin_batched asks for more than 64 KiB of LDS beyond
n = 1984 / 960 / 448): A = H diag(d) H / n with H the Sylvester Hadamard matrix of order n, so
A_ij = f(i xor j) with f = H d / n, every entry exact at the word's width and the spectrum d
exactly (d: integers below 2^20, multi-word plus 2^-60 times a second integer vector).

Measured on an MI355X, worst error / tolerance: dispatch table fp64 139 5.6e-5, 160 1.8e-4,
257 5.6e-5; dd 97 2.1e-4, 129 and 160 1.9e-4; qd 67 2.9e-13, 100 5.2e-4, 130 3.0e-13.  Scaled
(the same figure at 2^120, 2^-120, 2^600 and 2^-600): fp64 160 1.8e-4, dd 128 1.7e-6, qd 80
7.5e-4.  Hadamard: fp64 2048 0 (the exact integer), dd 1024 3.6e-6, qd 512 3.8e-16, dd 4096 1.4e-6 (2.5 s).  STEP stage,
chain against the default: fp64 delta = 160 lambda 5.2e-4, alpha 3.8e-4; dd delta = 100 9.9e-5
and 1.1e-4 of their bounds.
"""
import mpmath
import numpy as np
import pytest

import test_gpu_eigmin_sizes as es
import test_gpu_step_large as tsl

pytestmark = pytest.mark.gpu

BLK, BATCHED = 5, 4   # CLRSDP_EIG_K_BLK, CLRSDP_EIG_K_BATCHED (include/clrsdp.h)


def _tol(words, n):
    return 1e-12 * max(1.0, n / 128.0) if words == 1 else es.EIG_TOL[words] * max(1.0, n / 64.0)


def _check(pk, words, cases, label):
    """es._check with this file's tolerance: one clrsdp_eigmin call over ``cases`` =
    [(name, kind, n, exponent)], every lambda_min against the block's reference to _tol(words, n)
    of its spectral radius; prints the worst error / tolerance."""
    g = 30 if words == 1 else 60
    refs = [es._block(kind, n, g) for _, kind, n, _ in cases]
    got = pk.eigmin([es._for_words(r[0], words, c[3]) for r, c in zip(refs, cases)], precision_words=words)
    ratios, bad = [], []
    with mpmath.workprec(320):
        for (name, kind, n, ex), (_, lam, rad), gv in zip(cases, refs, got):
            gm = mpmath.mpf(float(gv)) if words == 1 else mpmath.mpf(gv)
            err = abs(mpmath.ldexp(gm, -ex) - lam) / rad
            ratio = float(err / _tol(words, n)) if mpmath.isfinite(err) else float("inf")
            ratios.append((ratio, name))
            if not ratio <= 1.0:
                bad.append((name, n, ex, str(gm), float(lam), ratio))
    w = max(ratios)
    print(f"eigmin {label}: {len(cases)} blocks, worst error / tolerance {w[0]:.3g} at {w[1]}")
    assert not bad, f"(block, n, exponent, lambda_min, reference, error / tolerance): {bad}"


@pytest.fixture
def chain(monkeypatch):
    monkeypatch.setenv("CLRSDP_EIG_BLK", "1")


CHAIN_SIZES = [(1, 139), (1, 160), (1, 257), (2, 97), (2, 129), (2, 160), (4, 67), (4, 100), (4, 130)]


@pytest.mark.parametrize("words,nmax", CHAIN_SIZES)
def test_chain_across_the_dispatch_table(pk, chain, words, nmax):
    """One clrsdp_eigmin call per (words, nmax), the batch of
    test_eigmin_across_the_dispatch_table, through the chain."""
    assert pk.eigmin_kernel(nmax, words) == BLK
    cases = [(f"{k}{nmax}", k, nmax, 0) for k in ("spread", "tiny", "triple", "cI", "decoupled", "2x2")]
    cases += [("rider1", "one", 1, 0), ("rider2", "two", 2, 0)]
    cases += [(f"rider{n}", "spread", n, 0) for n in (3, 17, 64)]
    _check(pk, words, cases, f"chain words={words} nmax={nmax}")


@pytest.mark.parametrize("ex", [120, -120, 600, -600])
@pytest.mark.parametrize("words,n", [(1, 160), (2, 128), (4, 80)])
def test_chain_scaled_blocks(pk, chain, words, n, ex):
    """The spread and decoupled blocks times 2^ex: the prepass divides the block by the power of
    two of its largest leading-limb magnitude (a max over the strips' partials) and eigblk_sturm
    multiplies lambda_min back."""
    assert pk.eigmin_kernel(n, words) == BLK
    cases = [(f"spread{n}", "spread", n, ex), (f"decoupled{n}", "decoupled", n, ex)]
    _check(pk, words, cases, f"chain words={words} n={n} scale=2^{ex}")


def _sym(rng, n):
    A = rng.standard_normal((n, n))
    return (A + A.T) / 2


@pytest.mark.parametrize("words,n,big", [(1, 150, 200), (2, 110, 140), (4, 75, 90)])
def test_chain_result_is_independent_of_the_grid(pk, chain, words, n, big):
    """The same block alone and as the third of a batch with a larger block: bitwise the same
    lambda_min (every p_i is one thread's ascending-column sum and every reflector is formed by
    the same instruction sequence in every workgroup; the grid of each launch follows the batch's
    nmax).  The strip height is a compile-time constant of the library, so it cannot be varied
    here: tools/micro/eig_blk_bench compares strips of 16, 32 and 64 rows bitwise."""
    rng = np.random.default_rng(4242 + words)
    A, B, S = _sym(rng, n), _sym(rng, big), _sym(rng, 70)
    assert pk.eigmin_kernel(n, words) == BLK and pk.eigmin_kernel(big, words) == BLK
    alone = pk.eigmin([A], precision_words=words)
    batch = pk.eigmin([B, S, A], precision_words=words)
    ref = float(np.linalg.eigvalsh(A)[0])
    rad = float(np.max(np.abs(np.linalg.eigvalsh(A))))
    err = abs(float(alone[0]) - ref) / rad
    print(f"grid independence words={words} n={n}: lambda_min {float(alone[0]):.17g}, "
          f"against numpy / (n eps) {err / (n * 2.2e-16):.3g}")
    assert err <= n * 2.2e-16    # numpy's own backward error: a sanity check, not the precision test
    assert alone[0] == batch[2], (alone[0], batch[2])


def _fwht(v):
    v = np.array(v, dtype=np.int64)
    h = 1
    while h < len(v):
        v = v.reshape(-1, 2, h)
        v = np.stack([v[:, 0] + v[:, 1], v[:, 0] - v[:, 1]], axis=1).reshape(-1)
        h *= 2
    return v


@pytest.mark.parametrize("words,n", [(1, 2048), (2, 1024), (4, 512), (2, 4096)])
def test_chain_past_the_one_cu_launch_request(pk, chain, words, n):
    """A_ij = f(i xor j), f = H d / n (module docstring): exact entries, spectrum d exactly.  The
    limbs are formed here (an error-free two-sum of f1 and 2^-60 f2) and go to clrsdp_eigmin as
    planes, without a million multi-word Python numbers on the way.  Double-double 4096, the
    largest block clrsdp_eigmin takes, is the one case in which eigblk_sturm reads the tridiagonal
    from global memory (2n words no longer fit beside the fp64 copy past n = 3410) and asks for
    more than 64 KiB of LDS."""
    from clrsdp_amd import _lib
    from clrsdp_amd.instance import from_planes
    assert pk.eigmin_kernel(n, words) == BLK
    rng = np.random.default_rng(900 + words)
    d1 = rng.integers(-2**20 + 1, 2**20, n)
    d2 = rng.integers(-2**20 + 1, 2**20, n) if words > 1 else np.zeros(n, dtype=np.int64)
    f1 = _fwht(d1).astype(np.float64) / n            # exact: |H d| < n 2^20, n a power of two
    f2 = np.ldexp(_fwht(d2).astype(np.float64) / n, -60)
    hi = f1 + f2
    lo = (f1 - (hi - (hi - f1))) + (f2 - (hi - f1))  # two-sum: hi + lo = f1 + f2 exactly
    idx = np.arange(n)[:, None] ^ np.arange(n)[None, :]
    planes = np.zeros((words, n * n))
    planes[0] = hi[idx].reshape(-1)
    if words > 1:
        planes[1] = lo[idx].reshape(-1)
    planes = planes.reshape(-1)
    out = np.zeros(words)
    nn = np.array([n], dtype=np.int64)
    _lib.check(_lib.lib().clrsdp_eigmin(0, words, 1, nn.ctypes.data_as(_lib.P_i64),
                                        planes.ctypes.data_as(_lib.P_f64), out.ctypes.data_as(_lib.P_f64)))
    with mpmath.workprec(320):
        lam = [mpmath.mpf(int(a)) + mpmath.ldexp(mpmath.mpf(int(b)), -60) for a, b in zip(d1, d2)]
        ref, rad = min(lam), max(abs(v) for v in lam)
        got = from_planes(out, 1, words)[0]
        ratio = float(abs(got - ref) / rad / _tol(words, n))
    print(f"eigmin chain hadamard words={words} n={n}: worst error / tolerance {ratio:.3g}")
    assert ratio <= 1.0, (float(got), float(ref), ratio)


def test_default_is_untouched(pk, monkeypatch):
    """With the switch unset, clrsdp_eigmin at fp64 160 takes eigmin_batched and returns bitwise
    what it returns with CLRSDP_EIG_BLK=0."""
    A = _sym(np.random.default_rng(160), 160)
    monkeypatch.delenv("CLRSDP_EIG_BLK", raising=False)
    assert pk.eigmin_kernel(160, 1) == BATCHED
    unset = pk.eigmin([A], precision_words=1)
    monkeypatch.setenv("CLRSDP_EIG_BLK", "0")
    assert pk.eigmin_kernel(160, 1) == BATCHED
    zero = pk.eigmin([A], precision_words=1)
    assert unset[0] == zero[0], (unset[0], zero[0])


# ---------------------------------------------------------------- through the solver

def _step_stage(pk, oracle, words, D, on, monkeypatch):
    """Scalars after STAGE_STEP (stages run one by one) on test_gpu_step_large's handle with X/Y
    blocks of D and 12, the switch on or unset when the handle is created."""
    from clrsdp_amd import _lib as L
    from clrsdp_amd import instance as inst
    if on:
        monkeypatch.setenv("CLRSDP_EIG_BLK", "1")
    else:
        monkeypatch.delenv("CLRSDP_EIG_BLK", raising=False)
    cons, b, bi, state = tsl._state(pk, oracle, D)
    P = pk.make_params("0.3", "0.1", tsl.GAMMA, 0)
    dev = pk.DeviceSolver(cons, b, pk.get_block_info(cons), precision_words=words)
    try:
        dev.set_state(*state)
        for s in range(L.STAGE_MU_R, L.STAGE_STEP + 1):
            dev.run_stage(s, P, False)
        _, X, _, Y = dev.get_state(True)
        dX = inst.flat_to_blocks(dev.buffer(L.BUF_DXMAT, True), bi)
        dY = inst.flat_to_blocks(dev.buffer(L.BUF_DYMAT, True), bi)
        sc = {k: dev.scalar(k, True) for k in ("mineig_X", "mineig_Y", "alpha_p", "alpha_d")}
    finally:
        dev.close()
    return bi, X, dX, Y, dY, sc


@pytest.mark.parametrize("words,D", [(1, 160), (2, 100)])
def test_step_stage_with_the_chain(pk, oracle, monkeypatch, words, D):
    """STAGE_STEP with the chain against the same stage with the switch unset: each lambda slot
    to tol(n) rad, rad the largest fp64 spectral radius of L_b^-1 dM_b L_b^-T over the blocks
    (both runs are within that of the true minimum; the stages before STEP launch the same
    kernels in both, so they see the same dM bitwise).  alpha = min(1, -gamma / lambda), so
    alpha_on - alpha_off = gamma (lambda_on - lambda_off) / (lambda_on lambda_off): to the same
    bound through that identity, plus one rounding of the word."""
    assert pk.eigmin_kernel(D, words) == BATCHED
    bi, X, dX, Y, dY, off = _step_stage(pk, oracle, words, D, False, monkeypatch)
    _, _, _, _, _, on = _step_stage(pk, oracle, words, D, True, monkeypatch)
    assert pk.eigmin_kernel(D, words) == BLK
    tol = _tol(words, D)
    eps = {1: 2.3e-16, 2: 2.5e-32}[words]
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
            print(f"step chain words={words} D={D} {lk}: {float(l1):.17g} against {float(l0):.17g}, "
                  f"error / tolerance {lerr:.3g}; {ak} {float(a1):.17g} against {float(a0):.17g}, "
                  f"error / bound {aerr:.3g}")
            worst = max(worst, lerr, aerr)
    assert worst <= 1.0, worst


def test_iterate_equals_the_stages_with_the_chain(pk, oracle, chain):
    """fp64, X/Y blocks of 160 and 12: clrsdp_iterate (the captured loop body, about 320 chain
    launches in it) leaves bitwise the state and scalars of the ten stages run one by one."""
    from clrsdp_amd import _lib as L
    from clrsdp_amd import instance as inst
    cons, b, bi, state = tsl._state(pk, oracle, 160)
    P = pk.make_params("0.3", "0.1", tsl.GAMMA, 0)
    got = []
    for whole in (False, True):
        dev = pk.DeviceSolver(cons, b, pk.get_block_info(cons), precision_words=1)
        try:
            dev.set_state(*state)
            if whole:
                dev.iterate(P, False)
            else:
                for s in range(L.STAGE_MU_R, L.STAGE_UPDATE + 1):
                    dev.run_stage(s, P, False)
            x, X, y, Y = dev.get_state()
            sc = np.asarray(dev.buffer(L.BUF_SCALARS), dtype=np.float64)
            got.append((np.asarray(x), inst.blocks_to_flat(X), np.asarray(y), inst.blocks_to_flat(Y),
                        sc[[L.SC[k] for k in ("mineig_X", "mineig_Y", "alpha_p", "alpha_d", "mu")]]))
        finally:
            dev.close()
    for name, a, c in zip(("x", "X", "y", "Y", "scalars"), got[0], got[1]):
        assert np.array_equal(a, c), name
    print(f"iterate against stages, chain on: mineig_X {got[1][4][0]:.17g}, alpha_p {got[1][4][2]:.17g}")
