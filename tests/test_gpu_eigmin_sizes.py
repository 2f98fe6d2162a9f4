"""lambda_min (clrsdp_eigmin) in every eigen-solver's size range, at each word width.

MatPlan<T>::eigmin (csrc/clrsdp.hip) picks the kernel from the batch's nmax and the word type.
From eig_lds_bytes (sizeof(T) (n^2 + 10 n + 40) for n > 64), eig2_lds_bytes
(sizeof(T) (n ld + 3 ld + 2 n + 20) + 64, ld = 16 ceil(n/16) + 8), LDS_MAX = 160 KiB and the
nmax <= 64 guards of eigmin_mx and of eigmin_lds2<qd>:

    words | kernel by nmax
    fp64  | eigmin_split <= 128; eigmin_lds 129-138; eigmin_batched >= 139
    dd    | eigmin_mx (+ eigmin_lds2 redo) <= 64; eigmin_lds2 65-93; eigmin_lds 94-96;
          | eigmin_batched >= 97
    qd    | eigmin_mx (+ redo) <= 64; eigmin_lds 65-66; eigmin_batched >= 67

(fp64: 138^2 + 1380 + 40 = 20464 <= 20480 < 20751 at 139.  dd: eigmin_lds2 93 -> 163104 B <=
163840 < 164800 B at 94; eigmin_lds 96 -> 10216 <= 10240 words < 10419 at 97.  qd: eigmin_lds
66 -> 5056 <= 5120 words < 5199 at 67.)  The sizes below sit on both sides of every boundary.

Each batch is one call: blocks of n = nmax with a known spectrum (helpers.known_spectrum, so
lambda_min = min(lam) with no eigen-solve) and closed-form raw structures, plus riders of n = 1,
2, 3, 17 and 64, which run inside the large-block kernel because nmax chooses it.

Tolerance, relative to the block's spectral radius max|lam_i|: multi-word, EIG_TOL[words] of
test_gpu_steplength.py times max(1, n/64) (the tridiagonalisation's backward error grows as
n eps ||T||); fp64, 1e-12 (TOL of test_gpu_steplength.py).  The limb split of the 320-bit entries
(at fp64: their rounding to binary64) moves lambda_min by at most n 2^-BITS ||A||, far inside both.

Scale: the same blocks times 2^+-120 and 2^+-600 (exact in every limb, so the reference scales
exactly), one size per kernel and width; clrsdp_eigmin's supported range is stated in
include/clrsdp.h.

Measured on an MI355X, worst error / tolerance of each batch (every test prints it): fp64 129
4.4e-4, 138 and 139 5.6e-5, 160 2.2e-4; dd 65 and 93 2.5e-4, 94 and 96 4.3e-4, 97 3.5e-4,
129 2.2e-4, 160 2.3e-4; qd 65 2.9e-13, 66 1.5e-3, 67 2.5e-14, 100 1.4e-14.  Scaled, the same
figure at 2^120, 2^-120, 2^600 and 2^-600 (the scaling is exact): fp64 138 1.2e-6, 160 2.2e-4; dd
40 3.3e-5, 80 1.4e-6, 96 5.9e-7, 128 7.6e-6; qd 40 8.4e-4, 66 1.5e-3, 80 6e-17.  Before the
kernels scaled their input, every 2^600 case returned NaN and every 2^-600 case the smallest
diagonal entry of the unreduced block (decoupled: 0.4999999999995 for 0.0005 .. 0.0056).
"""
import mpmath
import numpy as np
import pytest

from helpers import known_spectrum

pytestmark = pytest.mark.gpu

EIG_TOL = {2: 1e-28, 4: 1e-50}   # test_gpu_steplength.EIG_TOL


def _tol(words, n):
    return 1e-12 if words == 1 else EIG_TOL[words] * max(1.0, n / 64.0)


def _mp(x):
    with mpmath.workprec(320):
        return mpmath.mpf(x)


def _spectrum(kind, n, g):
    with mpmath.workprec(320):
        lin = lambda a, b, cnt: [_mp(a) + (_mp(b) - _mp(a)) * i / max(cnt - 1, 1) for i in range(cnt)]
        if kind == "spread":     # clustered minimum: -1/2, -1/2 + 2^-g, the rest in [-0.4, 0.4]
            lam = [_mp(-0.5), _mp(-0.5) + mpmath.ldexp(1, -g)] + lin(-0.4, 0.4, n - 2)
        elif kind == "tiny":     # tiny positive minimum
            lam = [mpmath.ldexp(_mp(1), -40)] + lin(1, 2, n - 1)
        else:                    # triple minimum
            lam = [_mp(-1)] * 3 + lin(0, 1, n - 3)
        return lam[:n]


def _tridiag(n, d, e):
    A = np.zeros((n, n))
    A[np.diag_indices(n)] = d
    i = np.arange(n - 1)
    A[i + 1, i] = A[i, i + 1] = e
    return A


_BLOCKS = {}


def _block(kind, n, g=60):
    """(block, lambda_min, spectral radius) of one unscaled test block, built once and shared by
    the word widths: an object array of 320-bit numbers (known spectra) or a float array (raw
    structures, whose entries are binary fractions)."""
    key = (kind, n, g if kind == "spread" else 0)
    if key in _BLOCKS:
        return _BLOCKS[key]
    with mpmath.workprec(320):
        if kind in ("spread", "tiny", "triple"):
            lam = _spectrum(kind, n, g)
            seed = 50000 + 7 * n + {"spread": 0, "tiny": 1, "triple": 2}[kind]
            out = (known_spectrum(n, lam, np.random.default_rng(seed)), min(lam), max(abs(v) for v in lam))
        elif kind == "cI":
            out = (np.eye(n) * 0.75, _mp(0.75), _mp(0.75))
        elif kind == "decoupled":
            # constant tridiagonal d = 1/2, e = 1/4 with one zero coupling in the middle: the halves
            # have eigenvalues 1/2 + 1/2 cos(k pi / (m + 1)), the longer one the smaller minimum
            e = np.full(n - 1, 0.25)
            e[n // 2 - 1] = 0.0
            c = mpmath.cos(mpmath.pi / (max(n // 2, n - n // 2) + 1)) / 2
            out = (_tridiag(n, 0.5, e), _mp(0.5) - c, _mp(0.5) + c)
        elif kind == "2x2":
            # [[a, b], [b, a]] blocks with zero couplings between them: a -+ b (n odd: and a)
            e = np.where(np.arange(n - 1) % 2 == 0, 0.125, 0.0)
            out = (_tridiag(n, 0.5, e), _mp(0.375), _mp(0.625))
        elif kind == "one":      # n = 1, an entry with lower limbs
            v = -_mp(2) / 3
            out = (np.array([[v]], dtype=object), v, -v)
        elif kind == "two":      # n = 2: a -+ b
            a, b = _mp(1) / 3, _mp(1) / 7
            out = (np.array([[a, b], [b, a]], dtype=object), a - b, a + b)
        else:
            raise KeyError(kind)
    _BLOCKS[key] = out
    return out


def _for_words(A, words, ex=0):
    """The block as clrsdp_eigmin takes it at ``words``, times 2^ex (exact): floats at fp64 (the
    320-bit entries rounded to binary64), else an object array of mpmath numbers."""
    if words == 1 or A.dtype != object:
        F = A if A.dtype != object else np.array([[float(v) for v in row] for row in A])
        F = np.ldexp(F, ex)
        if words == 1:
            return F
        return np.array([[mpmath.mpf(float(v)) for v in row] for row in F], dtype=object)
    if ex == 0:
        return A
    with mpmath.workprec(320):
        return np.array([[mpmath.ldexp(v, ex) for v in row] for row in A], dtype=object)


def _check(pk, words, cases, label):
    """One clrsdp_eigmin call over ``cases`` = [(name, kind, n, exponent)]; every lambda_min
    against the block's reference to _tol(words, n) of its spectral radius.  Prints the worst
    error / tolerance."""
    g = 30 if words == 1 else 60
    refs = [_block(kind, n, g) for _, kind, n, _ in cases]
    got = pk.eigmin([_for_words(r[0], words, c[3]) for r, c in zip(refs, cases)], precision_words=words)
    ratios, bad = [], []
    with mpmath.workprec(320):
        for (name, kind, n, ex), (_, lam, rad), gv in zip(cases, refs, got):
            gm = mpmath.mpf(float(gv)) if words == 1 else mpmath.mpf(gv)
            err = abs(mpmath.ldexp(gm, -ex) - lam) / rad
            ratio = float(err / _tol(words, n)) if mpmath.isfinite(err) else float("inf")
            ratios.append((ratio, name))
            if not ratio <= 1.0:
                bad.append((name, n, ex, float(mpmath.ldexp(gm, -ex)) if mpmath.isfinite(gm) else str(gm),
                            float(lam), ratio))
    w = max(ratios)
    print(f"eigmin {label}: {len(cases)} blocks, worst error / tolerance {w[0]:.3g} at {w[1]}")
    assert not bad, f"(block, n, exponent, lambda_min / 2^ex, reference, error / tolerance): {bad}"


SIZES = [(1, 129), (1, 138), (1, 139), (1, 160),
         (2, 65), (2, 93), (2, 94), (2, 96), (2, 97), (2, 129), (2, 160),
         (4, 65), (4, 66), (4, 67), (4, 100)]


@pytest.mark.parametrize("words,nmax", SIZES)
def test_eigmin_across_the_dispatch_table(pk, words, nmax):
    """One batch per (words, nmax): at n = nmax the spread spectrum with a clustered minimum
    (gap 2^-60, fp64 2^-30), a tiny positive minimum (2^-40 under [1, 2]), a triple minimum, c I,
    the decoupled constant tridiagonal and the alternating 2 x 2 blocks; riders of n = 1, 2
    (closed forms; they never enter the kernel's column loop) and 3, 17, 64 (spread spectrum)."""
    cases = [(f"{k}{nmax}", k, nmax, 0) for k in ("spread", "tiny", "triple", "cI", "decoupled", "2x2")]
    cases += [("rider1", "one", 1, 0), ("rider2", "two", 2, 0)]
    cases += [(f"rider{n}", "spread", n, 0) for n in (3, 17, 64)]
    _check(pk, words, cases, f"words={words} nmax={nmax}")


SCALE_SIZES = [(1, 138), (1, 160), (2, 40), (2, 80), (2, 96), (2, 128), (4, 40), (4, 66), (4, 80)]


@pytest.mark.parametrize("ex", [120, -120, 600, -600])
@pytest.mark.parametrize("words,n", SCALE_SIZES)
def test_eigmin_scaled_blocks_every_kernel(pk, words, n, ex):
    """The spread-spectrum block and the decoupled tridiagonal times 2^ex, one size per kernel and
    width (n = 40: eigmin_mx, whose clustered block goes to the eigmin_lds2 redo).  At 2^+-600 the
    squares of the entries leave the binary64 range: the kernels divide the block by the power of
    two of its largest leading-limb magnitude when they load it and multiply lambda_min back."""
    cases = [(f"spread{n}", "spread", n, ex), (f"decoupled{n}", "decoupled", n, ex)]
    _check(pk, words, cases, f"words={words} n={n} scale=2^{ex}")


def test_eig_mx_0_takes_effect_inside_one_process(pk, monkeypatch):
    """Two double-double blocks of n = 8, twice in one process.  With CLRSDP_EIG_MX unset the batch
    takes eigmin_mx, which reports a route (0 certified, 1 flagged) for every block; with
    CLRSDP_EIG_MX=0 the same call takes eigmin_lds2 for every block (route -1), although a
    multi-word call has already run under the default.  lambda_min of the two calls agrees to
    _tol(2, 8) of the block's spectral radius."""
    refs = [_block("spread", 8, 60), _block("tiny", 8)]
    blocks = [_for_words(r[0], 2) for r in refs]
    monkeypatch.delenv("CLRSDP_EIG_MX", raising=False)
    mx, routes_mx = pk.eigmin(blocks, precision_words=2, return_routes=True)
    monkeypatch.setenv("CLRSDP_EIG_MX", "0")
    lds2, routes_lds2 = pk.eigmin(blocks, precision_words=2, return_routes=True)
    print(f"eigmin EIG_MX unset / 0: routes {list(routes_mx)} / {list(routes_lds2)}")
    assert all(int(r) >= 0 for r in routes_mx), list(routes_mx)
    assert all(int(r) == -1 for r in routes_lds2), list(routes_lds2)
    with mpmath.workprec(320):
        for (_, lam, rad), a, b in zip(refs, mx, lds2):
            diff = abs(mpmath.mpf(a) - mpmath.mpf(b)) / rad
            print(f"  |difference| / radius {float(diff):.3g} (tolerance {_tol(2, 8):.3g})")
            assert diff <= _tol(2, 8), (float(diff), float(lam))
