"""GPU tests of the low-rank operators and block kernels on their own (clrsdp_apply_operator,
include/clrsdp.h): colsum_rhs, colsum_dot + tuple_aggregate and the strip chain's TRACE form
(RHS), scale_cols + the weighted-A GEMMs and the fused scaled GEMM (WEIGHTED), blk_sym_tiles and
blk_sym2 in every mode and on the m > 1 subset (SYM), vec_lin and diag_add through blk_lin (LIN),
on the three handle kinds of tests/oper_cases.py at words 1, 2 and 4; then, without the entry
point, the residuals of a non-PD integer state against the oracle, and the keep-residuals copies
of the pipelined loop.  Instances, operand classes, references, bounds and checks are those of
tests/oper_cases.py: the exact class must be the exact integer as a value, the generic class
within (ops + 2) u sum |terms| componentwise; every test asserts the route the library took, and
prints its largest error / bound.

tests/test_oper_host.py shows without a GPU that these checks reject a subtly wrong kernel."""
import numpy as np
import pytest

import oper_cases as oc
import reduce_cases as rc
from oracle import mpmp_oracle as O

pytestmark = pytest.mark.gpu

WORDS = list(oc.WORDS)
_cache = {}


@pytest.fixture(scope="module")
def handles(pk):
    """one handle per (kind, class, words[, C]), built on first use and closed with the module"""
    devs = {}

    def get(kind, cls, words, C=None):
        key = (kind, cls, words, C is not None)
        if key not in devs:
            inst = oc.instance(kind, cls, words)
            cons = inst.clusters()
            devs[key] = pk.DeviceSolver(cons, inst.b, pk.get_block_info(cons), precision_words=words,
                                        C_blocks=C)
            assert devs[key].n_blk == inst.lay.n_blk and devs[key].n_x == inst.lay.n_x
        return devs[key]
    yield get
    for d in devs.values():
        d.close()


def _ops(kind, cls, words):
    """(Z, d, a, base) and the references of RHS and WEIGHTED, computed once and left unchanged"""
    key = (kind, cls, words)
    if key not in _cache:
        inst = oc.instance(kind, cls, words)
        Z, d, a, base = inst.blocks(1), inst.tuples(2), inst.tuples(3, pairs=True), inst.blocks(4, cancel=False)
        if cls == "exact":
            assert oc.caps_ok(inst, Z, d, a, base)
        v = dict(Z=Z, d=d, a=a, base=base, rhs=oc.rhs_eval(inst, Z, d),
                 wa={f: oc.weighted_eval(inst, a, base, fused=f) for f in (False, True)})
        for x in (Z, d, a, base):
            x.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ---- RHS: the U = Z V product and direction_rhs_ -------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("cls", oc.CLASSES)
@pytest.mark.parametrize("kind", oc.KINDS)
def test_rhs(handles, kind, cls, words):
    """rhs = -d - Tr(A_* Z) of a non-symmetric Z taken as given: the sub-blocks above the block
    diagonal of a block with m > 1, which trace_A never reads, hold NaN"""
    v, lay = _ops(kind, cls, words), oc.layout(kind)
    Zg = v["Z"].copy()
    Zg[:, lay.unread_mask(upper=True)] = oc.NAN
    got, route = handles(kind, cls, words).apply_operator("rhs", blocks=Zg, tuples=v["d"])
    assert route == oc.ROUTE_RHS[(kind, words)], f"route {route}"
    ref, bnd = v["rhs"]
    ok, fig = oc.judge(cls, got, ref, bnd)
    print(f"OPER rhs {kind} {cls} words={words} route={route}: error / bound = {fig:.3e}")
    assert ok, f"rhs {kind} {cls} words={words}: error / bound {fig:.3e}"


# ---- WEIGHTED: weighted_A(dx, p_wA_dX, dX, 1.0) ---------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("cls", oc.CLASSES)
@pytest.mark.parametrize("kind", oc.KINDS)
def test_weighted(handles, kind, cls, words):
    """base + sum_i a_i A_i: the base below the block diagonal of a block with m > 1 is never
    read (NaN there); such a block comes out as its upper triangle mirrored, bitwise symmetric"""
    v, lay = _ops(kind, cls, words), oc.layout(kind)
    Bg = v["base"].copy()
    Bg[:, lay.unread_mask(upper=False)] = oc.NAN
    got, route = handles(kind, cls, words).apply_operator("weighted", blocks=Bg, tuples=v["a"])
    assert route == oc.ROUTE_WEIGHTED[(kind, words)], f"route {route}"
    ref, bnd = v["wa"][route == 0]
    ok, fig = oc.judge(cls, got, ref, bnd)
    print(f"OPER weighted {kind} {cls} words={words} route={route}: error / bound = {fig:.3e}")
    assert ok, f"weighted {kind} {cls} words={words}: error / bound {fig:.3e}"
    assert oc.mirrored_bitwise(lay, got)


# ---- SYM: blk_sym_tiles / blk_sym2 -----------------------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("only_m", [False, True], ids=["all", "only_m"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_sym(handles, mode, only_m, words):
    """every mode on the thirteen block sizes of the general kind (1 .. 129 in a grid sized for
    the largest) and on its middle subset of m > 1 blocks.  Mode 0 is bitwise symmetric and, the
    input being dyadic, (Z + Z^T) / 2 exactly (generic class: within u (|Z| + |Z^T|)); modes 1 and
    2 are bitwise the source entries; blocks outside the subset are untouched"""
    lay = oc.layout("general")
    dev = handles("general", "exact", words)
    worst = 0.0
    for cls in oc.CLASSES:
        X = oc.instance("general", cls, words).blocks(5, cancel=False)
        out0 = np.full_like(X, oc.NAN2)
        got, route = dev.apply_operator("sym", blocks=X, mode=mode, only_m=only_m, out=out0)
        assert route == (0 if (words == 1 and mode == 0 and not only_m) else 1), f"route {route}"
        exp, ref, touched = oc.sym_expect(lay, X, mode, only_m, X if mode != 2 else out0)
        assert touched.all() != only_m
        # outside the subset: the input (in place) or the pre-filled payload (mode 2), bitwise
        keep = X if mode != 2 else out0
        assert rc.bitwise(got[:, ~touched], keep[:, ~touched])
        if mode == 0:
            assert oc.all_bitwise_symmetric(lay, got, only_m)
            bnd = np.zeros(lay.n_blk)
            for (j, l) in lay.order:
                Ab = np.abs(lay.block(X[0], j, l))
                lay.block(bnd, j, l)[:] = oc.EPS[words] * (Ab + Ab.T)
            ok, fig = oc.judge(cls, got, ref, bnd, mask=touched)
            assert ok, f"sym mode 0 {cls} words={words} only_m={only_m}: error / bound {fig:.3e}"
            worst = max(worst, fig)
        else:
            assert rc.bitwise(got, exp), f"sym mode {mode} {cls} words={words} only_m={only_m}"
    print(f"OPER sym mode={mode} only_m={only_m} words={words}: error / bound = {worst:.3e}")


# ---- LIN: vec_lin and diag_add through blk_lin ------------------------------------------------------
@pytest.mark.parametrize("words", WORDS)
def test_lin(pk, handles, words):
    """the three forms the solver issues: a copy (the value; bitwise at fp64), out = A - B in place (exact on
    integers, 2 u (|A| + |B|) on generic data), the diagonal add alone with its scalar read from a
    device word and its multiplier (blocks of 1, 127, 128, 129: diag_add's 128 threads)"""
    from clrsdp_amd import _lib as L
    lay = oc.layout("general")
    dev = handles("general", "exact", words)
    diag = np.zeros(lay.n_blk, dtype=bool)
    for q in lay.order:
        off, n = lay.blocks[q][:2]
        diag[off + np.arange(n) * (n + 1)] = True
    worst = 0.0
    for cls in oc.CLASSES:
        inst = oc.instance("general", cls, words)
        A, B = inst.blocks(6, cancel=False), inst.blocks(7, cancel=False)
        got, route = dev.apply_operator("lin", blocks=A, mode=L.LIN_COPY)
        (Ia, ea), (Ib, eb) = rc.ints(A), rc.ints(B)
        # (vec_lin multiplies by T(1.0): a multi-word copy may renormalise the limbs -- the exact
        # class's planes at 2^-140 and 2^-190 fit one double -- but never changes the value)
        assert route == 0 and rc.value_equal(got, (Ia, ea)), f"copy {cls} words={words}"
        assert words > 1 or rc.bitwise(got, A), f"copy {cls} words={words}"
        got, _ = dev.apply_operator("lin", blocks=A, blocks2=B, mode=L.LIN_SUB)
        ref = rc.add((Ia, ea), (-Ib, eb))
        ok, fig = oc.judge(cls, got, ref, oc.lin_bound(words, A, B))
        assert ok, f"A - B {cls} words={words}: error / bound {fig:.3e}"
        worst = max(worst, fig)
        # A + (s mult) I
        if cls == "exact":
            s, mult = np.array([3.0, 2.0 ** -80, 2.0 ** -140, 2.0 ** -190][:words]), -2.0
        else:
            s, mult = rc.generic_vector(1, words, 9, cancel=False)[:, 0], 0.75
        got, _ = dev.apply_operator("lin", blocks=A, scalar=s, mult=mult, mode=L.LIN_DIAG)
        assert rc.bitwise(got[:, ~diag], A[:, ~diag]), f"diag_add wrote off the diagonal ({cls}, words={words})"
        sm = rc.scale(rc.ints(s), mult)
        ref = rc.add((Ia[diag], ea), (np.array([sm[0][0]] * int(diag.sum()), dtype=object), sm[1]))
        bnd = 2 * oc.EPS[words] * (np.abs(A[0, diag]) + abs(s[0] * mult))
        ok, fig = oc.judge(cls, got[:, diag], ref, bnd)
        assert ok, f"diag_add {cls} words={words}: error / bound {fig:.3e}"
        worst = max(worst, fig)
    print(f"OPER lin words={words}: error / bound = {worst:.3e}")


def test_apply_operator_refusals(pk, handles):
    from clrsdp_amd import _lib as L
    dev = handles("uniform", "exact", 1)
    lay = oc.layout("uniform")
    Z, d = np.zeros((1, lay.n_blk)), np.zeros((1, lay.n_x))
    for kw in (dict(op="rhs", blocks=Z), dict(op="rhs", tuples=d), dict(op="weighted", tuples=d),
               dict(op="sym", blocks=Z, mode=3), dict(op="lin", blocks=Z, mode=7),
               dict(op="lin", blocks=Z, mode=L.LIN_SUB), dict(op="lin", blocks=Z, mode=L.LIN_DIAG)):
        with pytest.raises(L.ClrsdpError) as e:
            dev.apply_operator(**kw)
        assert e.value.code == L.E_ARG, kw
    # refused while a loop body is in flight, and usable again after it
    cons, b = pk.synth(seed=3, J=2, delta=4, rank=1, n_y=3)
    bi = pk.get_block_info(cons)
    dev = pk.DeviceSolver(cons, b, bi)
    try:
        dev.set_state(*pk.initial_point(bi, 10.0, 10.0))
        prm = pk.make_params("0.3", "0.1", "0.7", 0)
        dev.initial_residuals(prm)
        dev.iterate_async(prm)
        Z = rc.generic_vector(dev.n_blk, 1, 5, cancel=False)
        with pytest.raises(L.ClrsdpError) as e:
            dev.apply_operator("lin", blocks=Z, mode=L.LIN_COPY)
        assert e.value.code == L.E_STATE
        dev.iterate_wait()
        got, _ = dev.apply_operator("lin", blocks=Z, mode=L.LIN_COPY)
        assert rc.bitwise(got, Z)
    finally:
        dev.close()


# ---- without the entry point: the residuals of a non-PD integer state ----------------------------
@pytest.mark.parametrize("words", WORDS)
@pytest.mark.parametrize("with_C", [False, True], ids=["noC", "C"])
@pytest.mark.parametrize("kind", oc.KINDS)
def test_initial_residuals_equal_the_oracle(pk, handles, kind, with_C, words):
    """set_state -> initial_residuals -> get_buffer(P, PVEC, DVEC) on one-limb integers (X and C
    symmetric, Y not, none of them definite): the general trace route (colsum_dot +
    tuple_aggregate) and weighted A (+ P - C through blk_lin) of every handle kind must give the
    integers of the oracle's compute_residuals, whose fp64 arithmetic is exact on them"""
    from clrsdp_amd import _lib as L
    inst = oc.instance(kind, "exact", words)
    lay = inst.lay
    cons = inst.clusters()
    bi = O.get_block_info(cons)
    blocks = lambda flat: [[lay.block(flat, j, l).copy() for l in range(bi.L[j])] for j in range(bi.J)]
    symm = lambda bl: [[b + b.T for b in bj] for bj in bl]
    x = inst.tuples(3)[0]
    X, Y = symm(blocks(inst.blocks(4)[0])), blocks(inst.blocks(1)[0])
    C = symm(blocks(inst.blocks(8)[0])) if with_C else None
    y = inst.b * 2.0
    P, p, d = O.compute_residuals(O.Fp64(), cons, x, X, y, Y, inst.b, C, bi, False)
    dev = handles(kind, "exact", words, C)
    dev.set_state(x, X, y, Y)
    dev.initial_residuals(pk.make_params("0.3", "0.1", "0.7", 0))
    for name, buf, ref in (("P", L.BUF_P, np.concatenate([P[j][l].reshape(-1, order="F") for (j, l) in lay.order])),
                           ("p", L.BUF_PVEC, p), ("d", L.BUF_DVEC, d)):
        got = dev.buffer(buf, exact=words > 1)
        bad = np.flatnonzero(np.asarray(got != ref, dtype=bool))
        assert bad.size == 0, f"{name} {kind} words={words}: {bad.size} entries differ, first at {bad[:5]}"
    assert np.max(np.abs(d)) < 2.0 ** 40 and max(np.max(np.abs(b)) for bj in P for b in bj) < 2.0 ** 40
    print(f"OPER residuals {kind} C={with_C} words={words}: P, p, d equal the oracle's integers")


# ---- the keep-residuals copies of the pipelined loop ------------------------------------------------
def test_pipelined_loop_keeps_the_last_residuals(pk):
    """fp64, one cluster with m = 1, delta = 3, N = 5: 9 block elements, 5 tuples, 3 free
    variables, all odd, so both segments of copy_guard2 end in an 8-byte tail.  Run to device-side
    termination, P, p and d are bitwise those of the synchronous loop's last body"""
    cons, b = pk.synth(J=1, delta=3, rank=1, n_y=3, seed=5, m=1, N=5)
    bi = pk.get_block_info(cons)
    assert bi.Y_blocksizes == [[3]] and bi.dim_S == [5]
    runs = []
    for pipelined in (False, True):
        res = pk.solverank1sdp(cons, b, bi, duality_gap_threshold="1e-8", primal_error_threshold="1e-8",
                               dual_error_threshold="1e-8", verbose=False, pipelined=pipelined,
                               return_info=True)
        runs.append(res)
        assert res[-1].status == "terminated", res[-1].status
    (s, q) = runs
    assert s[-1].iterations == q[-1].iterations
    for k, name in ((4, "P"), (5, "p"), (6, "d")):
        a = s[k][0][0] if name == "P" else s[k]
        c = q[k][0][0] if name == "P" else q[k]
        assert rc.bitwise(np.asarray(a), np.asarray(c)), f"{name}: pipelined {c} synchronous {a}"
    print(f"OPER keep-residuals: {s[-1].iterations} bodies, P, p, d bitwise equal")
