"""Host mirror of ``solverank1sdp`` (MPMP.jl:595-1025) driving the MI355X library.

The loop control, the termination test, the printed table and the returned 11-tuple follow
the reference exactly; every loop body (MPMP.jl:755-887) is one ``clrsdp_iterate`` call that
runs entirely on the GPU.  Numbers cross the boundary as planar limbs (``precision_words`` 1 =
fp64, 2 = double-double).
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .blockinfo import BlockInfo
from .instance import Flat, blocks_to_flat, concat_colmajor, flat_to_blocks, flatten, from_planes, \
    to_planes

DEFAULTS = dict(beta_infeasible="0.3", beta_feasible="0.1", gamma="0.7", omega_p="1e10",
                omega_d="1e10", duality_gap_threshold="1e-15", primal_error_threshold="1e-30",
                dual_error_threshold="1e-30")


def limbs(v, words=4):
    """A scalar (float, str, mpmath.mpf) as `words` limbs of an unevaluated sum."""
    import mpmath
    with mpmath.workprec(320):
        r = mpmath.mpf(v) if not isinstance(v, float) else mpmath.mpf(v)
        out = []
        for _ in range(words):
            h = float(r)
            out.append(h)
            r = r - h
    return out


def make_params(beta_infeasible, beta_feasible, gamma, b0) -> _lib.Params:
    p = _lib.Params()
    for name, v in (("beta_infeasible", beta_infeasible), ("beta_feasible", beta_feasible),
                    ("gamma", gamma), ("b0", b0)):
        arr = getattr(p, name)
        for i, x in enumerate(limbs(v)):
            arr[i] = x
    return p


def make_control(duality_gap_threshold, primal_error_threshold, dual_error_threshold,
                 need_primal_feasible=False, need_dual_feasible=False) -> _lib.Control:
    c = _lib.Control()
    for name, v in (("duality_gap_threshold", duality_gap_threshold),
                    ("primal_error_threshold", primal_error_threshold),
                    ("dual_error_threshold", dual_error_threshold)):
        arr = getattr(c, name)
        for i, x in enumerate(limbs(v)):
            arr[i] = x
    c.need_primal_feasible = 1 if need_primal_feasible else 0
    c.need_dual_feasible = 1 if need_dual_feasible else 0
    return c


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_lib.P_f64)


class DeviceSolver:
    """One handle of libclrsdp: constraint data resident on one GPU (the clusters of this rank)."""

    def __init__(self, constraints: Sequence, b, bi: BlockInfo, precision_words: int = 1,
                 C_blocks=None, device: int = 0, rank: int = 0, world: int = 1,
                 owned: Optional[Sequence[int]] = None, timing: bool = False):
        self.L = _lib.lib()
        self.bi = bi
        self.w = int(precision_words)
        self.rank, self.world = rank, world
        flat = flatten(constraints, bi)
        self.flat = flat
        self._keep = []
        desc = _lib.Desc()
        desc.J = bi.J
        desc.n_y = bi.n_y
        for name in ("m", "L", "n_samples", "delta", "ranks"):
            arr = np.ascontiguousarray(getattr(flat, name), dtype=np.int64)
            self._keep.append(arr)
            setattr(desc, name, arr.ctypes.data_as(_lib.P_i64))
        cfg = _lib.Config()
        cfg.precision_words = self.w
        cfg.device = device
        cfg.rank = rank
        cfg.world_size = world
        if owned is not None:
            own = np.ascontiguousarray(sorted(owned), dtype=np.int32)
            self._keep.append(own)
            cfg.owned = own.ctypes.data_as(_lib.P_i32)
            cfg.n_owned = len(own)
        cfg.timing = 1 if timing else 0
        self.timing = bool(timing)
        h = C.c_void_p()
        _lib.check(self.L.clrsdp_create(C.byref(desc), C.byref(cfg), C.byref(h)))
        self.h = h
        self.owned = sorted(owned) if owned is not None else list(range(bi.J))
        w = self.w
        Vp = to_planes(concat_colmajor(flat.V), w)
        lp = to_planes(np.concatenate(flat.lam), w)
        Bp = to_planes(concat_colmajor(flat.B), w)
        cp = to_planes(np.concatenate(flat.c), w)
        bp = to_planes(np.asarray(b), w)
        Cp = to_planes(blocks_to_flat(C_blocks), w) if C_blocks is not None else None
        self.check(self.L.clrsdp_upload_constraints(
            self.h, _ptr(Vp), _ptr(lp), _ptr(Bp), _ptr(cp), _ptr(bp),
            _ptr(Cp) if Cp is not None else None))
        self.n_x = sum(bi.dim_S)
        self.n_blk = sum(n * n for bj in bi.Y_blocksizes for n in bj)

    # ------------------------------------------------------------------ plumbing
    def check(self, rc):
        _lib.check(rc, self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.clrsdp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _from_planes(self, planes: np.ndarray, n: int, exact=False):
        if self.w == 1 or not exact:
            return planes[:n].copy()
        return from_planes(planes, n, self.w)

    # ------------------------------------------------------------------ state
    def set_state(self, x, X, y, Y):
        w = self.w
        xp = to_planes(np.asarray(x), w)
        Xp = to_planes(blocks_to_flat(X), w)
        yp = to_planes(np.asarray(y), w)
        Yp = to_planes(blocks_to_flat(Y), w)
        self.check(self.L.clrsdp_set_state(self.h, _ptr(xp), _ptr(Xp), _ptr(yp), _ptr(Yp)))

    def get_state(self, exact=False):
        w = self.w
        xp = np.zeros(w * self.n_x)
        Xp = np.zeros(w * self.n_blk)
        yp = np.zeros(w * self.bi.n_y)
        Yp = np.zeros(w * self.n_blk)
        self.check(self.L.clrsdp_get_state(self.h, _ptr(xp), _ptr(Xp), _ptr(yp), _ptr(Yp)))
        x = self._from_planes(xp, self.n_x, exact)
        y = self._from_planes(yp, self.bi.n_y, exact)
        X = flat_to_blocks(self._from_planes(Xp, self.n_blk, exact), self.bi)
        Y = flat_to_blocks(self._from_planes(Yp, self.n_blk, exact), self.bi)
        return x, X, y, Y

    def buffer(self, buf: int, exact=False) -> np.ndarray:
        cnt = C.c_int64()
        self.check(self.L.clrsdp_get_buffer(self.h, buf, None, C.byref(cnt)))
        n = cnt.value
        out = np.zeros(self.w * max(n, 1))
        self.check(self.L.clrsdp_get_buffer(self.h, buf, _ptr(out), C.byref(cnt)))
        return self._from_planes(out, n, exact)

    def global_P_d(self):
        """P (blocks) and d (vector) in the global layout of get_state: the device buffers hold
        the owned clusters only (in owned order); the other clusters' entries are zero, as in
        get_state, and live on the ranks that own them."""
        bi = self.bi
        Pl, dl = self.buffer(_lib.BUF_P), self.buffer(_lib.BUF_DVEC)
        if len(self.owned) == bi.J:
            return flat_to_blocks(Pl, bi), dl
        P = [[np.zeros((n, n)) for n in bj] for bj in bi.Y_blocksizes]
        d = np.zeros(self.n_x)
        xoff = np.concatenate([[0], np.cumsum(bi.dim_S)])
        po = lo = 0
        for j in self.owned:
            for l, n in enumerate(bi.Y_blocksizes[j]):
                P[j][l] = np.asarray(Pl[po:po + n * n]).reshape(n, n, order="F")
                po += n * n
            D = bi.dim_S[j]
            d[xoff[j]:xoff[j] + D] = dl[lo:lo + D]
            lo += D
        return P, d

    def scalar(self, name: str, exact=False):
        return self.buffer(_lib.BUF_SCALARS, exact)[_lib.SC[name]]

    def apply_operator(self, op: str, blocks=None, blocks2=None, tuples=None, scalar=None,
                       mult: float = 1.0, mode: int = 0, only_m: bool = False, out=None):
        """One of the handle's low-rank operators or block kernels on raw limbs
        (clrsdp_apply_operator).  ``op``: "rhs" (blocks = Z, tuples = d -> -d - Tr(A_* Z)),
        "weighted" (tuples = a, blocks = the base -> base + sum a_i A_i), "sym" (``mode`` 0, 1, 2,
        ``only_m``) or "lin" (``mode`` LIN_COPY, LIN_SUB with ``blocks2``, LIN_DIAG with ``scalar``
        (words limbs) and ``mult``).  Blocks are raw limbs of shape (words, n_blk) in the flat
        local layout of ``buffer``, tuples (words, n_x); ``out`` pre-fills the output (default:
        the payload).  Returns (raw limbs of the result, route).  The handle's work buffers are
        unspecified afterwards: call set_state before a loop body."""
        ops = {"rhs": _lib.APPLY_RHS, "weighted": _lib.APPLY_WEIGHTED, "sym": _lib.APPLY_SYM,
               "lin": _lib.APPLY_LIN}
        if op not in ops:
            raise ValueError("op: " + ", ".join(ops))
        if len(self.owned) != self.bi.J:
            raise ValueError("apply_operator: a handle that owns every cluster (the local layout "
                             "is then the global one)")
        w = self.w
        a = _lib.Operands()
        keep = []

        def limbs_of(v, n, what):
            if v is None:
                return None
            arr = _limbs2(v, w, what, n)
            keep.append(arr)
            return _ptr(arr)

        a.blocks = limbs_of(blocks, self.n_blk, "blocks")
        a.blocks2 = limbs_of(blocks2, self.n_blk, "blocks2")
        a.tuples = limbs_of(tuples, self.n_x, "tuples")
        a.scalar = limbs_of(None if scalar is None else np.asarray(scalar, dtype=np.float64).reshape(w, 1),
                            1, "scalar")
        a.mult, a.mode, a.only_m = float(mult), int(mode), 1 if only_m else 0
        nout = self.n_x if op == "rhs" else self.n_blk
        res = _payload((w, nout)).copy() if out is None else _limbs2(out, w, "out", nout).copy()
        if op == "rhs":
            a.tuples_out = _ptr(res)
        else:
            a.blocks_out = _ptr(res)
        route = C.c_int32(-1)
        self.check(self.L.clrsdp_apply_operator(self.h, ops[op], C.byref(a), C.byref(route)))
        return res, int(route.value)

    # ------------------------------------------------------------------ iteration
    def initial_residuals(self, prm: _lib.Params) -> _lib.IterStats:
        st = _lib.IterStats()
        self.check(self.L.clrsdp_initial_residuals(self.h, C.byref(prm), C.byref(st)))
        return st

    def iterate(self, prm: _lib.Params, pd_feas: bool) -> _lib.IterStats:
        st = _lib.IterStats()
        self.check(self.L.clrsdp_iterate(self.h, C.byref(prm), 1 if pd_feas else 0, C.byref(st)))
        return st

    def set_control(self, ctl: _lib.Control):
        self.check(self.L.clrsdp_set_control(self.h, C.byref(ctl)))

    def iterate_async(self, prm: _lib.Params):
        """Enqueue one loop body (pd_feas / termination decided on the device); no wait."""
        self.check(self.L.clrsdp_iterate_async(self.h, C.byref(prm)))

    def iterate_wait(self):
        """Stats of the oldest loop body in flight and whether it ran (0: the device had
        terminated before it)."""
        st = _lib.IterStats()
        ran = C.c_int32(0)
        self.check(self.L.clrsdp_iterate_wait(self.h, C.byref(st), C.byref(ran)))
        return st, bool(ran.value)

    def run_stage(self, stage: int, prm: _lib.Params, pd_feas: bool):
        self.check(self.L.clrsdp_run_stage(self.h, stage, C.byref(prm), 1 if pd_feas else 0))

    def synchronize(self):
        self.check(self.L.clrsdp_synchronize(self.h))

    def set_timing(self, on):
        """Per-stage HIP-event timing: False/0 off, True/1 every stage (no graph), 2 only the
        SCHUR stage, from device-clock stamps inside the replayed loop-body graph (off or 2 + one rank:
        iterate replays a hipGraph)."""
        mode = 2 if on == 2 else (1 if on else 0)
        self.check(self.L.clrsdp_set_timing(self.h, mode))
        self.timing = mode == 1

    def save_state(self):
        """Device-side snapshot of x, X, y, Y and the scalar slots (clrsdp_save_state)."""
        self.check(self.L.clrsdp_save_state(self.h))

    def restore_state(self):
        """Restore the last snapshot, stream-ordered after the work already enqueued."""
        self.check(self.L.clrsdp_restore_state(self.h))

    def handoff_state_to(self, other: "DeviceSolver"):
        """clrsdp_handoff_state: copy x, X, y, Y into ``other`` on the device; ``other`` may have
        another precision_words (wider: the limbs then zeros; narrower: the leading limbs) but
        needs the same description, device and owned clusters.  ``other`` is then as after
        ``set_state`` (call ``initial_residuals`` next) and this handle may be closed."""
        _lib.check(self.L.clrsdp_handoff_state(other.h, self.h), other.h)

    def set_factorization(self, flags: int):
        """clrsdp_set_factorization: FACT_FALLBACK (default: pivoted LU once a Cholesky fails),
        FACT_LU_SQ (S_j and Q by pivoted LU, the reference's approx_lu!), FACT_LU_X (X^-1 by
        approx_inv!)."""
        self.check(self.L.clrsdp_set_factorization(self.h, int(flags)))

    @property
    def factorization(self) -> int:
        f = C.c_int32(0)
        self.check(self.L.clrsdp_get_factorization(self.h, C.byref(f)))
        return f.value

    def set_graph(self, on: bool):
        """clrsdp_set_graph: hipGraph replay of the loop body on/off (off: eager enqueue)."""
        self.check(self.L.clrsdp_set_graph(self.h, 1 if on else 0))

    def comm_info(self):
        """(ranks, backend) of the exchange: backend 'none', 'rccl' (native communicator, ranks
        from ncclCommCount) or 'callback' (clrsdp_set_exchange)."""
        n, b = C.c_int32(0), C.c_int32(0)
        self.check(self.L.clrsdp_comm_info(self.h, C.byref(n), C.byref(b)))
        return n.value, {0: "none", 1: "rccl", 2: "callback"}.get(b.value, str(b.value))

    def schur_info(self) -> dict:
        """clrsdp_schur_info: what this handle's SCHUR stage launches, as a dict of ints -- fast,
        fused, one, d64, grp2, fused_y, n_fwg, n_ptiles, n_gsum, ozaki, pair_upper, and full /
        s_lower of the last SCHUR enqueued (-1 before any).  Read-only."""
        o = _lib.SchurInfo()
        self.check(self.L.clrsdp_schur_info(self.h, C.byref(o)))
        return {n: int(getattr(o, n)) for n, _ in _lib.SchurInfo._fields_}

    def set_stream(self, stream_ptr: int):
        self.check(self.L.clrsdp_set_stream(self.h, C.c_void_p(stream_ptr)))

    def stream_ptr(self) -> int:
        """The hipStream_t every launch of this handle goes to."""
        return self.L.clrsdp_get_stream(self.h) or 0

    def exchange_bytes(self) -> int:
        b = C.c_int64()
        self.check(self.L.clrsdp_exchange_bytes(self.h, C.byref(b)))
        return b.value

    def comm_init(self, uid: bytes):
        """Attach the native RCCL communicator (clrsdp_comm_init): every rank passes the id rank 0
        got from :func:`comm_unique_id`; the exchanges are then all-gathers issued by the
        library on its stream.  With one rank they are captured into the replayed loop-body
        graph; with more ranks the body is enqueued eagerly unless CLRSDP_GRAPH_RCCL=1."""
        if len(uid) != _lib.COMM_ID_BYTES:
            raise ValueError("RCCL unique id must be %d bytes" % _lib.COMM_ID_BYTES)
        self.check(self.L.clrsdp_comm_init(self.h, bytes(uid)))

    def set_exchange(self, fn, send_ptr: int, recv_ptr: int):
        self._xfn = _lib.EXCHANGE_FN(fn)
        self.check(self.L.clrsdp_set_exchange(self.h, self._xfn, None, C.c_void_p(send_ptr),
                                              C.c_void_p(recv_ptr)))


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id (clrsdp_comm_unique_id), to be created on rank 0 only."""
    buf = C.create_string_buffer(_lib.COMM_ID_BYTES)
    _lib.check(_lib.lib().clrsdp_comm_unique_id(buf))
    return buf.raw


def compute_step_length(M, dM, gamma, device: int = 0, return_eigs: bool = False):
    """compute_step_length(M, dM, gamma, blockinfo) of MPMP.jl:1829-1898 on the GPU (fp64,
    clrsdp_step_length): ``min(1, -gamma / lambda_min)`` over the blocks of L^-1 dM L^-T with
    M = L L^T.  ``M`` and ``dM`` are nested block lists (as X/Y) or flat lists of square
    arrays.  Returns ``(alpha, bigfloat_steplength)`` as the reference does (the flag is always
    False: there is no ball-arithmetic fallback), plus the per-block lambda_min with
    ``return_eigs``.  Raises ClrsdpError(E_STEP) when a block of M is not positive definite."""
    def flat(blocks):
        out = []
        for b in blocks:
            if isinstance(b, (list, tuple)):
                out.extend(flat(b))
            else:
                out.append(np.asarray(b, dtype=np.float64))
        return out
    Mb, dMb = flat(M), flat(dM)
    if len(Mb) != len(dMb) or not Mb:
        raise ValueError("M and dM need the same non-empty block structure")
    for a, b in zip(Mb, dMb):
        if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape != b.shape:
            raise ValueError("blocks must be square and M, dM blocks of equal size")
    n = np.array([a.shape[0] for a in Mb], dtype=np.int64)
    Mf = np.concatenate([a.ravel(order="F") for a in Mb])
    dMf = np.concatenate([b.ravel(order="F") for b in dMb])
    alpha = C.c_double(0.0)
    eig = np.zeros(len(Mb))
    _lib.check(_lib.lib().clrsdp_step_length(device, len(Mb), n.ctypes.data_as(_lib.P_i64),
                                              _ptr(Mf), _ptr(dMf), float(gamma), C.byref(alpha),
                                              _ptr(eig)))
    if return_eigs:
        return alpha.value, False, eig
    return alpha.value, False


def eigmin(blocks, precision_words: int = 1, device: int = 0, return_routes: bool = False):
    """lambda_min of each exactly symmetric block at fp64 / double-double / quad-double
    (clrsdp_eigmin; the eigenvalue part of compute_step_length, MPMP.jl:1857-1870).  Blocks are
    float arrays or object arrays of mpmath numbers (split exactly into limbs); returns floats
    (words 1) or mpmath numbers (the exact limb sums).  With ``return_routes`` (clrsdp_eigmin_routes)
    also one int per block: 0 certified by the refinement of eigmin_mx / the mxblk route, 1 flagged
    by it and computed by the fallback launch, -1 the batch's kernel has no certification step."""
    w = int(precision_words)
    mats = [np.asarray(b) for b in blocks]
    for a in mats:
        if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
            raise ValueError("blocks must be square")
    n = np.array([a.shape[0] for a in mats], dtype=np.int64)
    flat = np.concatenate([a.reshape(-1, order="F") for a in mats])
    planes = to_planes(flat, w)
    out = np.zeros(w * len(mats))
    routes = np.zeros(len(mats), dtype=np.int32)
    if return_routes:
        _lib.check(_lib.lib().clrsdp_eigmin_routes(device, w, len(mats), n.ctypes.data_as(_lib.P_i64),
                                                   _ptr(planes), _ptr(out),
                                                   routes.ctypes.data_as(C.POINTER(C.c_int32))))
    else:
        _lib.check(_lib.lib().clrsdp_eigmin(device, w, len(mats), n.ctypes.data_as(_lib.P_i64),
                                            _ptr(planes), _ptr(out)))
    eig = out if w == 1 else from_planes(out, len(mats), w)
    return (eig, routes) if return_routes else eig


def eigmin_kernel(nmax: int, precision_words: int = 1) -> int:
    """Which kernel ``eigmin`` (and the STEP stage's eigen launches) takes for a batch whose largest
    block is ``nmax``, under the current environment: one of ``_lib.EIG_K_*``
    (clrsdp_eigmin_kernel; a host-only query, no device and no launch).  ``EIG_K_MXBLK`` (6)
    stands in eigmin_batched's multi-word range with ``CLRSDP_EIG_MX_BLK=1`` (unless
    ``CLRSDP_EIG_MX=0``): the fp64 eigenpair refined at the word's width across workgroups, then
    the flagged blocks by the route the switch replaced."""
    k = C.c_int32(-1)
    _lib.check(_lib.lib().clrsdp_eigmin_kernel(int(precision_words), int(nmax), C.byref(k)))
    return k.value


def potrf_kernel(nmax: int, precision_words: int = 1) -> int:
    """Which kernel ``potrf`` without the inverse (and the FACTOR stage's Cholesky launches) takes
    for a batch whose largest block is ``nmax``, under the current environment
    (``CLRSDP_POTRF_BLK``): one of ``_lib.POTRF_K_*`` (clrsdp_potrf_kernel; a host-only query, no
    device and no launch).  It answers the route, not potrf_batched's size refusal."""
    k = C.c_int32(-1)
    _lib.check(_lib.lib().clrsdp_potrf_kernel(int(precision_words), int(nmax), C.byref(k)))
    return k.value


def spdinv_kernel(nmax: int, precision_words: int = 1, lu: bool = False) -> bool:
    """Whether the XINV stage / chol(Q) of a batch whose largest block is ``nmax`` form the
    inverse inside the factorisation's launch (True) or by a GEMM behind it, under the current
    environment (clrsdp_spdinv_kernel: fp64 and nmax <= 128 only, never with the LU fallback
    ``lu``; ``CLRSDP_CHOL_SPDINV=0`` keeps the GEMM).  A host-only query."""
    k = C.c_int32(-1)
    _lib.check(_lib.lib().clrsdp_spdinv_kernel(int(precision_words), int(nmax), 1 if lu else 0,
                                               C.byref(k)))
    return bool(k.value)


def chol_spdinv(blocks, want=None, pitch=None, fill=np.nan, device: int = 0):
    """``L^-1`` and, where ``want[b]``, ``A^-1 = L^-T L^-1`` of fp64 symmetric positive definite
    blocks (n <= 128) from one launch of the factorisation kernel (clrsdp_chol_spdinv).  ``want``:
    one flag per block (default: every block); ``pitch``: per block the leading dimension of both
    outputs (default n).  Returns ``(Linv, Ainv, info)``: per block two arrays of shape
    (pitch, n) that held ``fill`` in every entry before the launch, so what the kernel did not
    write still holds it, and ``info`` as ``potrf(inverse=True)``."""
    mats = [np.asarray(b, dtype=np.float64) for b in blocks]
    for a in mats:
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("blocks must be square")
    n = np.array([a.shape[0] for a in mats], dtype=np.int64)
    ld = n.copy() if pitch is None else np.array(pitch, dtype=np.int64)
    w = np.ones(len(mats), dtype=np.int32) if want is None else \
        np.array([1 if f else 0 for f in want], dtype=np.int32)
    if len(ld) != len(mats) or len(w) != len(mats):
        raise ValueError("one pitch and one flag per block")
    A = np.ascontiguousarray(np.concatenate([a.reshape(-1, order="F") for a in mats]))
    tot = max(int((ld * n).sum()), 1)
    Li = np.full(tot, fill, dtype=np.float64)
    Gi = np.full(tot, fill, dtype=np.float64)
    info = np.zeros(max(len(mats), 1), dtype=np.int32)
    _lib.check(_lib.lib().clrsdp_chol_spdinv(device, len(mats), n.ctypes.data_as(_lib.P_i64),
                                             ld.ctypes.data_as(_lib.P_i64),
                                             w.ctypes.data_as(_lib.P_i32), _ptr(A), _ptr(Li),
                                             _ptr(Gi), info.ctypes.data_as(_lib.P_i32)))
    off = np.concatenate([[0], np.cumsum(ld * n)])
    cut = lambda v, b: v[off[b]:off[b + 1]].reshape((ld[b], n[b]), order="F").copy()
    return ([cut(Li, b) for b in range(len(mats))], [cut(Gi, b) for b in range(len(mats))],
            info[:len(mats)].copy())


def getrf(blocks, precision_words: int = 1, device: int = 0, raw_limbs: bool = False):
    """Partially pivoted LU of each square block, ``A[perm] = L U``, at fp64 / double-double /
    quad-double (clrsdp_getrf: approx_lu!, MPMP.jl:1436, 1501, as the solver's LU path runs it).
    Blocks are float arrays or object arrays of mpmath numbers (split exactly into limbs).
    Returns ``(LU, perms, info)``: per block the factors in one matrix (L unit, below the
    diagonal; U on and above it; floats at words 1, else the exact limb sums as mpmath numbers),
    ``perm[k]`` = original row at position k (0-based), and ``info`` = 0 or the 1-based column
    of the first zero pivot.  With ``raw_limbs`` the factors come back as the raw limbs instead,
    one float array of shape (words, n, n) per block."""
    w = int(precision_words)
    mats = [np.asarray(b) for b in blocks]
    for a in mats:
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("blocks must be square")
    n = np.array([a.shape[0] for a in mats], dtype=np.int64)
    flat = np.concatenate([a.reshape(-1, order="F") for a in mats]) if mats else np.zeros(0)
    planes = np.ascontiguousarray(to_planes(flat, w), dtype=np.float64).copy()
    perm = np.zeros(max(int(n.sum()), 1), dtype=np.int32)
    info = np.zeros(max(len(mats), 1), dtype=np.int32)
    _lib.check(_lib.lib().clrsdp_getrf(device, w, len(mats), n.ctypes.data_as(_lib.P_i64),
                                       _ptr(planes), perm.ctypes.data_as(_lib.P_i32),
                                       info.ctypes.data_as(_lib.P_i32)))
    off = np.concatenate([[0], np.cumsum(n * n)])
    poff = np.concatenate([[0], np.cumsum(n)])
    if raw_limbs:
        P = planes.reshape(w, -1)
        LU = [P[:, off[b]:off[b + 1]].reshape((w, n[b], n[b])).transpose(0, 2, 1).copy()
              for b in range(len(mats))]
    else:
        vals = planes if w == 1 else from_planes(planes, flat.size, w)
        LU = [vals[off[b]:off[b + 1]].reshape((n[b], n[b]), order="F") for b in range(len(mats))]
    perms = [perm[poff[b]:poff[b + 1]].copy() for b in range(len(mats))]
    return LU, perms, info[:len(mats)].copy()


def potrf(blocks, inverse: bool = False, precision_words: int = 1, device: int = 0,
          raw_limbs: bool = False):
    """Cholesky factor ``A = L L^T`` of each symmetric positive definite block at fp64 /
    double-double / quad-double (clrsdp_potrf: cho!, as the solver's potrf plan runs it), or with
    ``inverse`` its inverse ``L^-1`` (the on-chip factorisation with the inverse: n <= 256 at
    fp64, n <= 64 at multi-word).  Without ``inverse`` the one-CU ``potrf_batched`` factors fp64
    blocks and quad-double blocks above 64, and refuses n > 1262 / n > 302 (``CLRSDP_E_ARG``);
    ``CLRSDP_POTRF_BLK`` is three-state: unset or ``0`` that default with its refusals, explicitly
    on (``=1``) a blocked chain across workgroups in its place (fp64 at every n, quad-double above
    64, double-double as by default) with no size bound up to 4096.  Blocks are float arrays, object arrays of mpmath numbers (split
    exactly into limbs) or raw limbs of shape (words, n, n); only their lower triangles are used.
    Returns ``(L, info)``: per block the lower triangle of the result (``np.tril``: floats at
    words 1, else the exact limb sums as mpmath numbers) and ``info`` = 0 or the 1-based column of
    the first pivot that is not positive (fp64 with ``inverse``: the first column of its
    16-column tile); a failed block's contents are unspecified.  With ``raw_limbs`` the whole
    blocks come back as the device left them, one float array of shape (words, n, n) each."""
    w = int(precision_words)
    planes, n = [], []
    for a in blocks:
        a = np.asarray(a)
        if a.dtype != object and a.ndim == 3:      # raw limbs
            if a.shape[0] != w:
                raise ValueError("raw limbs need shape (words, n, n)")
            if a.shape[1] != a.shape[2]:
                raise ValueError("blocks must be square")
            pl = np.stack([a[q].reshape(-1, order="F") for q in range(w)]).astype(np.float64)
        else:
            if a.ndim != 2 or a.shape[0] != a.shape[1]:
                raise ValueError("blocks must be square")
            pl = np.asarray(to_planes(a.reshape(-1, order="F"), w), dtype=np.float64).reshape(w, -1)
        planes.append(pl)
        n.append(a.shape[-1])
    n = np.array(n, dtype=np.int64)
    A = np.ascontiguousarray(np.concatenate(planes, axis=1)) if planes else np.zeros((w, 0))
    info = np.zeros(max(len(planes), 1), dtype=np.int32)
    _lib.check(_lib.lib().clrsdp_potrf(device, w, 1 if inverse else 0, len(planes),
                                       n.ctypes.data_as(_lib.P_i64), _ptr(A),
                                       info.ctypes.data_as(_lib.P_i32)))
    off = np.concatenate([[0], np.cumsum(n * n)])
    out = []
    for b in range(len(planes)):
        seg = A[:, off[b]:off[b + 1]]
        if raw_limbs:
            out.append(seg.reshape((w, n[b], n[b])).transpose(0, 2, 1).copy())
        elif w == 1:
            out.append(np.tril(seg[0].reshape((n[b], n[b]), order="F")))
        else:
            vals = from_planes(np.ascontiguousarray(seg).reshape(-1), int(n[b] * n[b]), w)
            out.append(np.tril(np.asarray(vals, dtype=object).reshape((n[b], n[b]), order="F")))
    return out, info[:len(planes)].copy()


def trsm(blocks, rhs, mode: int, trans: bool, precision_words: int = 1, device: int = 0,
         raw_limbs: bool = False):
    """Triangular solves ``op(T_b) X_b = B_b`` of each block at fp64 / double-double / quad-double
    (clrsdp_trsm: approx_solve_tril! / approx_solve_triu!, as the solver's TrsmPlan runs them).
    ``mode`` 0: the block holds a lower triangular L (potrf's); 1: the unit lower L of getrf's
    factors; 2: their U, read transposed.  ``trans`` False solves L x = b (mode 2: U^T x = b),
    True solves L^T x = b (mode 2: U x = b).  Blocks and right-hand sides (n x nrhs, or vectors of
    length n) are float arrays, object arrays of mpmath numbers (split exactly into limbs) or raw
    limbs of shape (words, n, n) / (words, n, nrhs).  Returns the solutions, one array per block
    (floats at words 1, else the exact limb sums as mpmath numbers; with ``raw_limbs`` float
    arrays of shape (words, n, nrhs))."""
    w = int(precision_words)

    def planes_of(a, vec_ok):
        a = np.asarray(a)
        if a.dtype != object and a.ndim == 3:      # raw limbs
            if a.shape[0] != w:
                raise ValueError("raw limbs need shape (words, rows, columns)")
            return a.shape[1:], np.stack([a[q].reshape(-1, order="F") for q in range(w)]).astype(np.float64)
        if vec_ok and a.ndim == 1:
            a = a.reshape(-1, 1)
        if a.ndim != 2:
            raise ValueError("blocks and right-hand sides must be matrices")
        return a.shape, np.asarray(to_planes(a.reshape(-1, order="F"), w), dtype=np.float64).reshape(w, -1)

    if len(blocks) != len(rhs):
        raise ValueError("one right-hand side per block")
    As, Bs, n, nr = [], [], [], []
    for a, b in zip(blocks, rhs):
        sa, pa = planes_of(a, False)
        sb, pb = planes_of(b, True)
        if sa[0] != sa[1]:
            raise ValueError("blocks must be square")
        if sb[0] != sa[0]:
            raise ValueError("right-hand sides need as many rows as their block")
        As.append(pa); Bs.append(pb); n.append(sa[0]); nr.append(sb[1])
    n = np.array(n, dtype=np.int64)
    nr = np.array(nr, dtype=np.int64)
    A = np.ascontiguousarray(np.concatenate(As, axis=1)) if As else np.zeros((w, 0))
    B = np.ascontiguousarray(np.concatenate(Bs, axis=1)) if Bs else np.zeros((w, 0))
    _lib.check(_lib.lib().clrsdp_trsm(device, w, int(mode), 1 if trans else 0, len(As),
                                      n.ctypes.data_as(_lib.P_i64), nr.ctypes.data_as(_lib.P_i64),
                                      _ptr(A), _ptr(B)))
    off = np.concatenate([[0], np.cumsum(n * nr)])
    out = []
    for b in range(len(As)):
        seg = B[:, off[b]:off[b + 1]]
        if raw_limbs:
            out.append(seg.reshape((w, nr[b], n[b])).transpose(0, 2, 1).copy())
        elif w == 1:
            out.append(seg[0].reshape((n[b], nr[b]), order="F").copy())
        else:
            vals = from_planes(np.ascontiguousarray(seg).reshape(-1), int(n[b] * nr[b]), w)
            out.append(np.asarray(vals, dtype=object).reshape((n[b], nr[b]), order="F"))
    return out


# what gemm() and gemm_chain() put wherever a kernel must not write (a quiet NaN with a payload)
GEMM_PAYLOAD = np.uint64(0x7FF8C0DEC0DEC0DE)
_GEMM_FORMS = {"plain": _lib.GEMM_PLAIN, "sym": _lib.GEMM_SYM, "upper": _lib.GEMM_UPPER,
               "scaled": _lib.GEMM_SCALED, "mixed": _lib.GEMM_MIXED}


def _payload(shape):
    return np.full(shape, GEMM_PAYLOAD, dtype=np.uint64).view(np.float64)


def _limbs3(a, w, what):
    """a matrix as raw limbs (w, rows, cols): float 2-D (trailing limbs 0), object 2-D of mpmath
    numbers (split exactly), or raw limbs already"""
    a = np.asarray(a)
    if a.dtype != object and a.ndim == 3:
        if a.shape[0] != w:
            raise ValueError(f"{what}: raw limbs need shape (words, rows, columns)")
        return np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2:
        raise ValueError(f"{what}: matrices expected")
    pl = np.asarray(to_planes(a.reshape(-1, order="F"), w), dtype=np.float64).reshape(w, -1)
    return pl.reshape((w, a.shape[1], a.shape[0])).transpose(0, 2, 1)


@dataclass
class GemmResult:
    C: list            # per problem the M x N result (see gemm)
    path: int          # the kernel (_lib.PATH_*)
    untouched: bool    # every cell of the C arena outside the results still holds GEMM_PAYLOAD


def gemm(A, B, Cin=None, precision_words: int = 1, form: str = "plain", transa: bool = False,
         transb: bool = False, alpha: float = 1.0, beta: float = 0.0, dscal=None, dmult: float = 0.0,
         ops=None, sa=None, sl=None, inplace=False, ldpad: int = 0, gaps=None, device: int = 0,
         raw_limbs: bool = False) -> GemmResult:
    """One batched product launch ``C_p = alpha op(A_p) op(B_p) + beta Cin_p`` through the solver's
    GemmPlan (clrsdp_gemm, include/clrsdp.h).  ``A``, ``B`` (and ``Cin``) are lists of stored
    matrices: float arrays, object arrays of mpmath numbers, or raw limbs (words, rows, columns).
    ``form``: "plain", "sym", "upper", "scaled" (with the lists ``sa``, ``sl`` of K factors each) or
    "mixed" (``ops[p] = (transa, transb, alpha, beta, diag)``).  ``inplace`` (a bool, or one per
    problem): C starts as Cin and is updated in place; otherwise Cin is an arena of its own.

    Layout.  Every arena holds the problems one after the other with leading dimension rows +
    ``ldpad``; ``gaps[arena][p]`` ("A", "B", "C", "Cin") extra elements in front of problem p (equal
    shapes at equal gaps make a uniform batch).  The padding rows of A, B and Cin hold NaN.  The C
    arena has 64 guard elements at each end and holds GEMM_PAYLOAD in the guards, gaps, padding
    rows and (unless in place) the result cells, so a cell the kernel did not write is a NaN.

    Returns a :class:`GemmResult`; ``C[p]`` is a float array at words 1, else the exact limb sums
    as mpmath numbers (``raw_limbs``: float limbs (words, M, N) as the device left them)."""
    w = int(precision_words)
    if form not in _GEMM_FORMS:
        raise ValueError(f"unknown form {form!r}")
    P = len(A)
    if P == 0 or len(B) != P:
        raise ValueError("one B per A, at least one problem")
    mixed = form == "mixed"
    if mixed and (ops is None or len(ops) != P):
        raise ValueError("mixed: one (transa, transb, alpha, beta, diag) per problem")
    if form == "scaled" and (sa is None or sl is None or len(sa) != P or len(sl) != P):
        raise ValueError("scaled: one sa and one sl per problem")
    if Cin is not None and len(Cin) != P:
        raise ValueError("one Cin per problem")
    inpl = list(inplace) if isinstance(inplace, (list, tuple)) else [bool(inplace)] * P
    if len(inpl) != P or (any(inpl) and Cin is None):
        raise ValueError("inplace: one flag per problem, and Cin to start from")
    gaps = gaps or {}
    G = 64
    recs = (_lib.GemmProblem * P)()
    arenas = {k: [] for k in ("A", "B", "C", "Cin")}
    pos = {"A": 0, "B": 0, "C": G, "Cin": 0}
    arenas["C"].append(_payload((w, G)))
    cells = []

    def place(name, lim, fill):
        """append the (w, rows, cols) matrix with padded columns; returns (offset, ld)"""
        g = int(gaps.get(name, [0] * P)[p])
        if g:
            arenas[name].append(fill((w, g)))
        rows, cols = lim.shape[1:]
        ld = rows + ldpad
        buf = fill((w, cols, ld))
        buf[:, :, :rows] = lim.transpose(0, 2, 1)
        arenas[name].append(buf.reshape(w, -1))
        off = pos[name] + g
        pos[name] = off + ld * cols
        return off, ld

    nanfill = lambda shape: np.full(shape, np.nan)
    svec = []
    for p in range(P):
        a, b = _limbs3(A[p], w, "A"), _limbs3(B[p], w, "B")
        ta, tb = (bool(ops[p][0]), bool(ops[p][1])) if mixed else (bool(transa), bool(transb))
        M, K = (a.shape[2], a.shape[1]) if ta else (a.shape[1], a.shape[2])
        Kb, N = (b.shape[2], b.shape[1]) if tb else (b.shape[1], b.shape[2])
        if K != Kb:
            raise ValueError(f"problem {p}: op(A) is {M} x {K} but op(B) is {Kb} x {N}")
        r = recs[p]
        r.M, r.N, r.K = M, N, K
        r.offa, r.lda = place("A", a, nanfill)
        r.offb, r.ldb = place("B", b, nanfill)
        c0 = None
        if Cin is not None and Cin[p] is not None:
            c0 = _limbs3(Cin[p], w, "Cin")
            if c0.shape[1:] != (M, N):
                raise ValueError(f"problem {p}: Cin must be {M} x {N}")
        start = c0 if (inpl[p] and c0 is not None) else _payload((w, M, N))
        r.offc, r.ldc = place("C", start, _payload)
        cells.append((r.offc, r.ldc, M, N))
        r.offcin, r.ldcin = -1, r.ldc
        if c0 is not None and not inpl[p]:
            r.offcin, r.ldcin = place("Cin", c0, nanfill)
        if mixed:
            r.transa, r.transb, r.alpha, r.beta, r.diag = int(ta), int(tb), float(ops[p][2]), \
                float(ops[p][3]), int(bool(ops[p][4]))
        if form == "scaled":
            va, vl = np.asarray(sa[p], dtype=np.float64).ravel(), np.asarray(sl[p], dtype=np.float64).ravel()
            if len(va) != K or len(vl) != K:
                raise ValueError(f"problem {p}: sa and sl need K = {K} entries")
            r.offs = sum(len(v[0]) for v in svec)
            svec.append((va, vl))
    arenas["C"].append(_payload((w, G)))
    cat = lambda name: np.ascontiguousarray(np.concatenate(arenas[name], axis=1)) if arenas[name] else None
    Aa, Ba, Ca, Cia = cat("A"), cat("B"), cat("C"), cat("Cin")
    sav = np.ascontiguousarray(np.concatenate([v[0] for v in svec])) if svec else None
    slv = np.ascontiguousarray(np.concatenate([v[1] for v in svec])) if svec else None
    ds = None if dscal is None else np.array([float(dscal)])
    path = C.c_int32(0)
    opt = lambda a: None if a is None else _ptr(a)
    _lib.check(_lib.lib().clrsdp_gemm(
        device, w, _GEMM_FORMS[form], int(bool(transa)), int(bool(transb)), float(alpha), float(beta),
        opt(ds), float(dmult), P, recs, _ptr(Aa), Aa.shape[1], _ptr(Ba), Ba.shape[1], _ptr(Ca),
        Ca.shape[1], opt(Cia), 0 if Cia is None else Cia.shape[1], opt(sav), opt(slv),
        0 if sav is None else len(sav), C.byref(path)))
    mask = np.zeros(Ca.shape[1], dtype=bool)
    out = []
    for off, ld, M, N in cells:
        idx = (off + np.arange(M)[:, None] + ld * np.arange(N)[None, :])
        mask[idx.ravel()] = True
        lim = Ca[:, idx]                                   # (w, M, N)
        if raw_limbs:
            out.append(lim.copy())
        elif w == 1:
            out.append(lim[0].copy())
        else:
            vals = from_planes(np.ascontiguousarray(lim.reshape(w, -1)).reshape(-1), M * N, w)
            out.append(np.asarray(vals, dtype=object).reshape(M, N))
    untouched = bool(np.all(Ca.view(np.uint64)[:, ~mask] == GEMM_PAYLOAD))
    return GemmResult(out, int(path.value), untouched)


def gemm_chain(form: str, A1, B1, A2=None, C1=None, a1: float = 1.0, b1: float = 0.0, dot=None,
               halves: int = 1, lam=None, din=None, c_agg: float = 1.0, c_in: float = 0.0,
               device: int = 0):
    """One chain_f64 launch through the solver's ChainPlan (clrsdp_gemm_chain, include/clrsdp.h),
    fp64, lists of n x n float blocks (n <= 128), all of one size.
      "chain": ``O_p = A2_p (a1 A1_p B1_p + b1 C1_p)``; ``dot = (DA, DdA, DB)`` (lists of blocks)
               adds the dot epilogue.  Returns ``(O, partials)``: the per-workgroup partial sums of
               ``<DA + DdA, DB + O>`` in launch order (None without ``dot``).
      "sym":   ``O_p = L_p (a1 M_p L_p^T)`` with ``A1 = M`` and ``B1 = L`` lower triangular with
               exact zeros above the diagonal (the kernel relies on them); ``halves = 2``: the
               second half of the lists goes to the kernel as its second pointer set.  Returns
               ``(O, None)``.
      "trace": ``rout[p][t] = c_agg lam[p][t] ((A1_p B1_p)[:, t] . B1_p[:, t]) + c_in din[p][t]``,
               ``B1_p`` n x ncols; ``din`` may be None.  Returns ``(rout, None)``.
    O and rout start as GEMM_PAYLOAD, so an entry the kernel did not write comes back a NaN."""
    forms = {"chain": _lib.CHAIN, "sym": _lib.CHAIN_SYM, "trace": _lib.CHAIN_TRACE}
    if form not in forms:
        raise ValueError(f"unknown form {form!r}")
    mats = [np.asarray(a, dtype=np.float64) for a in A1]
    if not mats or any(a.ndim != 2 or a.shape != mats[0].shape or a.shape[0] != a.shape[1] for a in mats):
        raise ValueError("A1: square blocks of one size")
    n, tot = mats[0].shape[0], len(mats)
    if halves not in (1, 2) or tot % halves:
        raise ValueError("halves: 1 or 2, dividing the number of blocks")
    flat = lambda lst: np.ascontiguousarray(np.concatenate(
        [np.asarray(a, dtype=np.float64).reshape(-1, order="F") for a in lst]))

    def blocks(lst, what, cols=n):
        if lst is None or len(lst) != tot:
            raise ValueError(f"{what}: one block per problem")
        for a in lst:
            if np.asarray(a).shape != (n, cols):
                raise ValueError(f"{what}: blocks must be {n} x {cols}")
        return flat(lst)

    opt = lambda a: None if a is None else _ptr(a)
    a1v = flat(mats)
    if form == "trace":
        if B1 is None or len(B1) != tot or np.asarray(B1[0]).ndim != 2:
            raise ValueError("B1: one n x ncols block per problem")
        nc = np.asarray(B1[0]).shape[1]
        b1v = blocks(B1, "B1", nc)
        def vec(lst, what):
            if lst is None or len(lst) != tot or any(np.asarray(v).size != nc for v in lst):
                raise ValueError(f"{what}: ncols numbers per problem")
            return np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in lst]))

        lamv = vec(lam, "lam")
        dinv = None if din is None else vec(din, "din")
        rout = _payload(tot * nc).copy()
        _lib.check(_lib.lib().clrsdp_gemm_chain(
            device, forms[form], n, tot, 1, nc, float(a1), float(b1), _ptr(a1v), _ptr(b1v), None, None,
            None, None, None, None, None, _ptr(lamv), opt(dinv), float(c_agg), float(c_in), _ptr(rout)))
        return [rout[p * nc:(p + 1) * nc].copy() for p in range(tot)], None
    b1v, a2v = blocks(B1, "B1"), blocks(A2 if A2 is not None else (B1 if form == "sym" else None), "A2")
    c1v = None if C1 is None or form == "sym" else blocks(C1, "C1")
    O = _payload(tot * n * n).copy()
    dv, part = [None] * 3, None
    if dot is not None:
        if form != "chain" or len(dot) != 3:
            raise ValueError("dot = (DA, DdA, DB), with the chain form only")
        dv = [blocks(d, "dot") for d in dot]
        part = _payload(tot * (-(-n // 32))).copy()
    _lib.check(_lib.lib().clrsdp_gemm_chain(
        device, forms[form], n, tot // halves, halves, 0, float(a1), float(b1), _ptr(a1v), _ptr(b1v),
        opt(c1v), _ptr(a2v), _ptr(O), opt(dv[0]), opt(dv[1]), opt(dv[2]), opt(part), None, None, 0.0,
        0.0, None))
    return [O[p * n * n:(p + 1) * n * n].reshape((n, n), order="F").copy() for p in range(tot)], part


_RED_KINDS = {"flat_fold": _lib.RED_FLAT_FOLD, "flat_tree": _lib.RED_FLAT_TREE, "vec": _lib.RED_VEC,
              "fold": _lib.RED_FOLD, "ordered": _lib.RED_ORDERED}
_RED_OPS = {"dot": _lib.OP_DOT, "dotsum": _lib.OP_DOTSUM, "sum": _lib.OP_SUM, "max": _lib.OP_MAX,
            "min": _lib.OP_MIN, "maxabs": _lib.OP_MAXABS}


def _limbs2(a, w, what, n=None):
    """raw limbs (w, n) of a vector as a contiguous float64 array (a 1-D float vector: trailing
    limbs 0); bits are kept, NaN payloads included"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = np.concatenate([a[None], np.zeros((w - 1, a.size))])
    if a.ndim != 2 or a.shape[0] != w or (n is not None and a.shape[1] != n):
        raise ValueError(f"{what}: raw limbs of shape (words, {'n' if n is None else n}) expected")
    return np.ascontiguousarray(a)


def reduce(kind: str, a, b=None, da=None, db=None, op: str = "dot", stride: int = 1, folds=None,
           n=None, precision_words: int = 1, device: int = 0, return_partials: bool = False):
    """One of the solver's scalar reductions on raw limbs (clrsdp_reduce).  ``a`` (and ``b``,
    ``da``, ``db``) are float arrays of shape (words, n), or 1-D at words 1.  ``kind``:
    "flat_fold" / "flat_tree" (ops dot, dotsum, maxabs), "vec" (dot, maxabs), "ordered" (min over
    the ``n`` values ``a[:, i * stride]``) or "fold" with ``folds`` = up to 12 tuples
    (cnt, stride, off, op) over the arena ``a`` (ops sum, max, min, maxabs).  Returns the limbs of
    the result, shape (words,) (fold: (words, len(folds))); with ``return_partials`` (flat kinds)
    also the flat_reduce partials, shape (words, RED_G)."""
    w = int(precision_words)
    if kind not in _RED_KINDS:
        raise ValueError("kind: " + ", ".join(_RED_KINDS))
    av = _limbs2(a, w, "a")
    na = av.shape[1]
    opt = lambda v: None if v is None else _ptr(v)
    bv, dav, dbv = (None if v is None else _limbs2(v, w, nm, na)
                    for v, nm in ((b, "b"), (da, "da"), (db, "db")))
    fl, nfold, nout = None, 0, 1
    if kind == "fold":
        if not folds:
            raise ValueError("fold: a list of (cnt, stride, off, op)")
        nfold = nout = len(folds)
        fl = (_lib.Fold * nfold)()
        for q, (cnt, st, off, o) in enumerate(folds):
            if o not in _RED_OPS:
                raise ValueError("op: " + ", ".join(_RED_OPS))
            fl[q].cnt, fl[q].stride, fl[q].off, fl[q].op = int(cnt), int(st), int(off), _RED_OPS[o]
        ncall = na
    else:
        if op not in _RED_OPS:
            raise ValueError("op: " + ", ".join(_RED_OPS))
        ncall = na if kind != "ordered" else (int(n) if n is not None else (na - 1) // int(stride) + 1)
        if kind == "ordered" and (ncall - 1) * int(stride) + 1 != na:
            raise ValueError("ordered: a holds (n - 1) * stride + 1 numbers")
    out = _payload((w, nout)).copy()
    part = _payload((w, _lib.RED_G)).copy() if return_partials else None
    _lib.check(_lib.lib().clrsdp_reduce(device, w, _RED_KINDS[kind], _RED_OPS.get(op, -1), ncall,
                                        int(stride), _ptr(av), opt(bv), opt(dav), opt(dbv), nfold, fl,
                                        _ptr(out), opt(part)))
    res = out if kind == "fold" else out[:, 0]
    return (res, part) if return_partials else res


def slab_sum(slabs, n: int, base=None, cbase: float = 0.0, csum: float = 1.0, Q=None, out2: bool = False,
             guard: int = 0, precision_words: int = 1, device: int = 0):
    """out[e] = sum_i slabs[i, e] for e < n through slab_sum4, or with ``Q`` (fp64, n x n or ldq x n
    with ldq > n, column j in ``Q[:, j]``) Q times that sum through slab_qsolve (clrsdp_slab_sum).
    ``slabs`` has shape (words, cnt, stride) with stride >= n (2-D at words 1); ``base`` (words, n)
    gives cbase * base + csum * sum.  The outputs carry ``guard`` payload numbers on either side.
    Returns the raw output arrays, shape (words, n + 2 * guard): out, or (out, out2)."""
    w = int(precision_words)
    sl = np.asarray(slabs, dtype=np.float64)
    if sl.ndim == 2:
        sl = np.concatenate([sl[None], np.zeros((w - 1,) + sl.shape)])
    if sl.ndim != 3 or sl.shape[0] != w:
        raise ValueError("slabs: shape (words, cnt, stride)")
    cnt, stride = sl.shape[1:]
    sl = np.ascontiguousarray(sl.reshape(w, cnt * stride))
    bv = None if base is None else _limbs2(base, w, "base", int(n))
    qv, ldq = None, 0
    if Q is not None:
        Qm = np.asarray(Q, dtype=np.float64)
        if Qm.ndim != 2 or Qm.shape[1] != n or Qm.shape[0] < n:
            raise ValueError("Q: ldq x n with ldq >= n")
        ldq = Qm.shape[0]
        qv = np.ascontiguousarray(Qm.reshape(-1, order="F"))
    nout = int(n) + 2 * int(guard)
    out = _payload((w, nout)).copy()
    o2 = _payload((w, nout)).copy() if out2 else None
    _lib.check(_lib.lib().clrsdp_slab_sum(device, w, cnt, stride, int(n), _ptr(sl),
                                          None if bv is None else _ptr(bv), float(cbase), float(csum),
                                          None if qv is None else _ptr(qv), ldq, _ptr(out),
                                          None if o2 is None else _ptr(o2), nout, int(guard)))
    return (out, o2) if out2 else out


def update_state(X, dX, Y, dY, x, dx, c, y, dy, b, info, alpha=None, eig=None, gamma=None,
                 pd_feas: bool = False, precision_words: int = 1, device: int = 0):
    """One update_state launch on raw limbs of shape (words, n) (clrsdp_update_state).  ``alpha`` =
    (alpha_p, alpha_d), ``words`` limbs each: the slot path; or ``eig`` = (eigX, eigY), limbs of
    shape (words, nblk), with ``gamma`` (``words`` limbs) and ``pd_feas``: the fused path.  ``info``
    are the status words.  Returns a dict of the raw limbs the launch leaves: X, Y, x, y, part
    (words, 3, RED_G), and on the fused path step (words, 4) = min eigX, min eigY, alpha_p,
    alpha_d."""
    w = int(precision_words)
    Xv, Yv = (_limbs2(v, w, nm).copy() for v, nm in ((X, "X"), (Y, "Y")))
    nel = Xv.shape[1]
    dXv, dYv = _limbs2(dX, w, "dX", nel), _limbs2(dY, w, "dY", nel)
    xv = _limbs2(x, w, "x").copy()
    nx = xv.shape[1]
    dxv, cv = _limbs2(dx, w, "dx", nx), _limbs2(c, w, "c", nx)
    yv = _limbs2(y, w, "y").copy()
    ny = yv.shape[1]
    dyv, bv = _limbs2(dy, w, "dy", ny), _limbs2(b, w, "b", ny)
    iv = np.ascontiguousarray(info, dtype=np.int32)
    part = _payload((w, 3 * _lib.RED_G)).copy()
    lim = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(w))
    al = eg = gm = step = None
    nblk = 0
    if (alpha is None) == (eig is None):
        raise ValueError("either alpha (the slot path) or eig (the fused path)")
    if alpha is not None:
        al = [lim(alpha[0]), lim(alpha[1])]
    else:
        eg = [_limbs2(eig[0], w, "eigX"), _limbs2(eig[1], w, "eigY")]
        nblk = eg[0].shape[1]
        if eg[1].shape[1] != nblk:
            raise ValueError("eigX and eigY: one value per block each")
        gm = lim(gamma)
        step = _payload((w, 4)).copy()
    opt = lambda v: None if v is None else _ptr(v)
    xo = lambda v: _ptr(v) if nx else None
    _lib.check(_lib.lib().clrsdp_update_state(
        device, w, nel, _ptr(Xv), _ptr(dXv), _ptr(Yv), _ptr(dYv), nx, xo(xv), xo(dxv), xo(cv), ny,
        _ptr(yv), _ptr(dyv), _ptr(bv), iv.size, iv.ctypes.data_as(_lib.P_i32),
        opt(al and al[0]), opt(al and al[1]), nblk, opt(eg and eg[0]), opt(eg and eg[1]), opt(gm),
        1 if pd_feas else 0, _ptr(part), opt(step)))
    res = dict(X=Xv, Y=Yv, x=xv, y=yv, part=part.reshape(w, 3, _lib.RED_G))
    if step is not None:
        res["step"] = step
    return res


def cl_solve(Linv, W, rhs, dy, guard=None, device: int = 0):
    """The fp64 cluster solve in its two launches (clrsdp_cl_solve): per cluster c the D_c x D_c
    ``Linv[c]`` (lower triangle read), the D_c x ny ``W[c]`` and ``rhs[c]``; ``dy`` of ny numbers.
    t, the partial slabs and dx are pre-filled with ``guard`` (default: the payload).  Returns
    (t, slabs, dx): t and dx as lists per cluster, slabs of shape (ncl, nrb, ny)."""
    D = np.ascontiguousarray([np.asarray(l).shape[0] for l in Linv], dtype=np.int64)
    ncl, ny = len(D), int(np.asarray(dy).size)
    nrb = max(1, -(-int(D.max()) // 64)) if ncl else 1
    cat = lambda ms: np.ascontiguousarray(np.concatenate(
        [np.asarray(m, dtype=np.float64).reshape(-1, order="F") for m in ms])) if ncl else np.zeros(1)
    Lf, Wf, rf = cat(Linv), cat(W), cat(rhs)
    dyv = np.ascontiguousarray(dy, dtype=np.float64)
    nx = int(D.sum())
    fill = (lambda n: _payload((n,)).copy()) if guard is None else (lambda n: np.full(n, float(guard)))
    t, slabs, dx = fill(max(nx, 1)), fill(max(ncl * nrb * ny, 1)), fill(max(nx, 1))
    _lib.check(_lib.lib().clrsdp_cl_solve(device, ncl, D.ctypes.data_as(_lib.P_i64), ny, _ptr(Lf),
                                          _ptr(Wf), _ptr(rf), _ptr(dyv), _ptr(t), _ptr(slabs),
                                          _ptr(dx)))
    off = np.concatenate([[0], np.cumsum(D)])
    split = lambda v: [v[off[c]:off[c + 1]].copy() for c in range(ncl)]
    return split(t), slabs[:ncl * nrb * ny].reshape(ncl, nrb, ny), split(dx)


def initial_point(bi: BlockInfo, omega_p, omega_d):
    """x = 0, X = omega_p I, y = 0, Y = omega_d I (MPMP.jl:660-686)."""
    x = np.zeros(sum(bi.dim_S))
    X = [[float(omega_p) * np.eye(n) for n in bj] for bj in bi.Y_blocksizes]
    y = np.zeros(bi.n_y)
    Y = [[float(omega_d) * np.eye(n) for n in bj] for bj in bi.Y_blocksizes]
    return x, X, y, Y


def device_threshold(v, words):
    """A threshold as the device holds it at `words` limbs (clrsdp_set_control sums the first
    `words` limbs of :func:`limbs` in the word type, exactly): a float at fp64, else the exact
    mpmath value, so host comparisons at dd/qd are the device's own."""
    lv = limbs(v)
    if words == 1:
        return lv[0]
    import mpmath
    s = mpmath.mpf(0)
    for x in lv[:words]:
        s = mpmath.fadd(s, x, exact=True)
    return s


def _terminate(gap, perr, derr, gthr, pthr, dthr, need_p, need_d, out):
    """MPMP.jl:1147-1173."""
    gap_opt, pf, df = gap < gthr, perr < pthr, derr < dthr
    if need_p and pf:
        out("Primal feasible solution found")
        return True
    if need_d and df:
        out("Dual feasible solution found")
        return True
    if pf and df and gap_opt:
        out("Optimal solution found")
        return True
    return False


def log_row(it, t, st, p_obj, d_obj, dual_gap):
    """One row of the iteration table (MPMP.jl:923-937).  Every column is a float (the leading
    double of the device's value) except the gap, which is the loop control's own value: a float
    at fp64, the full-width mpmath number at dd/qd (the value terminate() compared, MPMP.jl:
    942-945, 1147-1173); the other columns at full width are in RunInfo.exact (record_exact)."""
    gap = dual_gap if not isinstance(dual_gap, (float, int, np.floating)) else float(dual_gap)
    return (int(it), float(t), float(st.mu), float(p_obj), float(d_obj), gap,
            float(st.P_err), float(st.p_err), float(st.d_err), float(st.alpha_p),
            float(st.alpha_d), float(st.beta_c))


HEADER = "%5s %8s %11s %11s %11s %10s %10s %10s %10s %10s %10s %10s" % (
    "iter", "time(s)", "μ", "P-obj", "D-obj", "gap", "P-error", "p-error", "d-error", "α_p",
    "α_d", "beta")


@dataclass
class RunInfo:
    iterations: int
    log: list
    phase_ms: np.ndarray
    time_total: float
    time_loop_after2: float
    status: str
    exact: list = None   # per iteration, the device scalar slots at full precision (record_exact)
    factorization: int = 1  # clrsdp_get_factorization at the end (an LU fallback adds its flag)
    lu_switch: int = 0      # iteration whose loop body switched to LU (0: none)
    inner_ms: np.ndarray = None  # the reference's inner buckets summed from iteration 3 (ms)
    # solve_escalating: per width (words, first iteration, bodies, reason), reason one of floor,
    # stalled, failed:<code>, terminated, maxiterations (empty for solverank1sdp)
    stages: list = field(default_factory=list)


def _stage_groups(ph):
    """The reference's timing groups (MPMP.jl:888-898) from the device stages (seconds)."""
    S = {n: ph[i] for i, n in enumerate(_lib.STAGE_NAMES)}
    return {"Decomp": S["schur"] + S["factor"], "predict_dir": S["predictor"],
            "correct_dir": S["corrector"], "alpha": S["step"], "Xinv": S["Xinv"],
            "R": S["mu_R"] + S["corrector_R"], "res": S["residuals"], "update": S["update"]}


def _first_iteration_times(ph):
    g = _stage_groups(ph)
    return ("decomp:%s. directions:%s. steplength:%s\nschur:%s factor (chol S, CinvB, Q, chol Q):%s\n"
            "X inv:%s. R:%s. residuals p,P,d:%s" % (
                g["Decomp"], g["predict_dir"] + g["correct_dir"], g["alpha"], ph[2], ph[3],
                g["Xinv"], g["R"], g["res"]))


def _time_spent(total, ph, inner=None):
    """MPMP.jl:973-1012.  Per-stage device times (sums over iterations 3, 4, ...) need the
    handle's HIP-event timing (DeviceSolver(timing=True)); without it only the total is known."""
    cols = ["total", "Decomp", "predict_dir", "correct_dir", "alpha", "Xinv", "R", "res"]
    lines = ["\nTime spent: (The total time may include compile time. The first few iterations "
             "are not included in the rest of the times)",
             ("%11s " * len(cols)).rstrip() % tuple(cols)]
    if ph is None:
        lines.append("%11.5e %s" % (total, "(per-stage times need DeviceSolver(timing=True))"))
        return "\n".join(lines) + "\n"
    g = _stage_groups(ph)
    lines.append(("%11.5e " * len(cols)).rstrip() % tuple([total] + [g[c] for c in cols[1:]]))
    if inner is None:
        lines.append("\nTime inside decomp:\n%11s %11s\n%11.5e %11.5e" % (
            "schur", "factor", ph[2], ph[3]))
        return "\n".join(lines) + "\n"
    # MPMP.jl:997-1012: the inner buckets (clrsdp_iter_stats.inner_ms, device time of each
    # bucket's launches; the direction buckets summed over predictor and corrector)
    lines.append("\nTime inside decomp:")
    lines.append(("%11s " * 5).rstrip() % ("schur", "chol_S", "comp CinvB", "comp Q", "chol_Q"))
    lines.append(("%11.5e " * 5).rstrip() % tuple(inner[:5]))
    lines.append("\nTime inside search directions (both predictor & corrector step)")
    lines.append(("%11s " * 5).rstrip() % ("calc Z", "calc rhs x", "solve system", "calc dX",
                                          "calc dY"))
    lines.append(("%11.5e " * 5).rstrip() % tuple(inner[5:10]))
    return "\n".join(lines) + "\n"


# a loop body that failed this way applied no update (the device guards the state update by the
# status words), so the state before it can be handed to a wider handle (solve_escalating)
STAGE_FAIL_CODES = (_lib.E_NOT_PD_X, _lib.E_NOT_PD_S, _lib.E_NOT_PD_Q, _lib.E_STEP)


class _Loop:
    """The loop control of ``solverank1sdp`` (MPMP.jl:720-1025 around the loop body): the values
    terminate() looks at, the log, the timers and the returned tuple.  ``solverank1sdp`` drives
    one handle with it, ``solve_escalating`` one handle per width, one after the other."""

    def __init__(self, prm_v, b0, need_primal_feasible, need_dual_feasible, out, testing,
                 record_exact):
        self.prm_v, self.b0, self.b0f = prm_v, b0, float(b0)
        self.need_p, self.need_d = need_primal_feasible, need_dual_feasible
        self.out, self.testing, self.record_exact = out, testing, record_exact
        self.it = 1
        self.log = []
        self.phase = np.zeros(_lib.NUM_STAGES)
        self.inner = np.zeros(_lib.NUM_INNER)
        self.t_start = None
        self.t_after2 = None
        self.status = "maxiterations"
        self.exact = []
        self.lu_switch = 0
        self.history = []   # the gap of every state a body of the current handle produced

    def attach(self, dev):
        """Loop control at the state's full width (MPMP.jl:942-945, 1067-1078, 1147-1185 run at
        the working precision): at dd/qd the thresholds are the device's exact multi-word values
        and the gap, errors and pd_feas are the device's own control_update results (all limbs),
        so a threshold below fp64 resolution is decided at the word's precision, and the
        synchronous and pipelined loops decide alike."""
        self.dev = dev
        self.exact_ctl = dev.w > 1
        self.gthr = device_threshold(self.prm_v["duality_gap_threshold"], dev.w)
        self.pthr = device_threshold(self.prm_v["primal_error_threshold"], dev.w)
        self.dthr = device_threshold(self.prm_v["dual_error_threshold"], dev.w)
        self.fact_seen = dev.factorization
        self.timed = bool(getattr(dev, "timing", False))
        self.history = []

    def device_control(self, st):
        """(gap, primal error, dual error) of the device's control_update for the state after
        the body `st` reports, all limbs (exact mpmath sums)."""
        import mpmath
        w = self.dev.w

        def v(limbs_):
            r = mpmath.mpf(0)
            for x in list(limbs_)[:w]:
                r = mpmath.fadd(r, x, exact=True)
            return r
        return v(st.gap_w), max(v(st.P_err_w), v(st.p_err_w)), v(st.d_err_w)

    def start(self, st, handed_over=False):
        """From the stats of initial_residuals.  The gap of the initial point excludes b0
        (compute_duality_gap(constraints, x, y, Y, C, b), MPMP.jl:725, 1067-1074); a state handed
        over from a narrower handle is an iterate of the running loop, whose gap includes it
        (MPMP.jl:942)."""
        b0f = self.b0f
        self.p_obj, self.d_obj = p_obj, d_obj = st.p_obj, st.d_obj
        if handed_over:
            self.dual_gap = abs(p_obj - d_obj) / max(1.0, abs(p_obj + d_obj))
        else:
            self.dual_gap = abs((p_obj - b0f) - (d_obj - b0f)) / max(1.0, abs((p_obj - b0f) + (d_obj - b0f)))
        self.perr = max(st.p_err, st.P_err)
        self.derr = st.d_err
        if self.exact_ctl:
            self.dual_gap, self.perr, self.derr = self.device_control(st)
            if handed_over:
                import mpmath
                with mpmath.workprec(64 * self.dev.w + 64):
                    sc = self.dev.buffer(_lib.BUF_SCALARS, exact=True)
                    pp, dd_ = +sc[_lib.SC["p_obj"]], +sc[_lib.SC["d_obj"]]
                    self.dual_gap = abs(pp - dd_) / max(mpmath.mpf(1), abs(pp + dd_))
        self.pd_feas = self.perr < self.pthr and self.derr < self.dthr
        if self.t_start is None:
            self.t_start = time.time()

    def record(self, st):
        dev, out = self.dev, self.out
        f = dev.factorization
        if f != self.fact_seen:   # the device switched to LU for the rest of the solve
            if (f & ~self.fact_seen) & _lib.FACT_LU_X:
                out("The inverse of X could not be computed with the cholesky factorization. We "
                    "switch to using the LU decomposition.")
            if (f & ~self.fact_seen) & _lib.FACT_LU_SQ:
                out("The Cholesky factorization of S or Q failed. We switch to the pivoted LU "
                    "decomposition (approx_lu!) for S and Q.")
            self.fact_seen = f
            self.lu_switch = self.lu_switch or self.it
        if self.it > 2:
            self.phase[:] += np.array(st.phase_ms[:])
            self.inner[:] += np.array(st.inner_ms[:])
        elif self.testing and self.timed:  # MPMP.jl:899-920: the times of the first iterations
            out(_first_iteration_times(np.array(st.phase_ms[:]) / 1e3))
        row = log_row(self.it, time.time() - self.t_start, st, self.p_obj, self.d_obj, self.dual_gap)
        self.log.append(row)
        out("%5d %8.1f %11.3e %11.3e %11.3e %10.2e %10.2e %10.2e %10.2e %10.2e %10.2e %10.2e" % row)
        self.p_obj, self.d_obj = st.p_obj, st.d_obj
        if self.exact_ctl:   # the device's full-width values (dd/qd)
            self.dual_gap, self.perr, self.derr = self.device_control(st)
        else:
            self.dual_gap = abs(self.p_obj - self.d_obj) / max(1.0, abs(self.p_obj + self.d_obj))  # MPMP.jl:942
            self.perr = max(st.p_err, st.P_err)                                # MPMP.jl:943
            self.derr = st.d_err
        self.it += 1
        self.pd_feas = self.perr < self.pthr and self.derr < self.dthr         # MPMP.jl:949-953
        self.history.append(self.dual_gap)

    def term(self):
        return _terminate(self.dual_gap, self.perr, self.derr, self.gthr, self.pthr, self.dthr,
                          self.need_p, self.need_d, self.out)

    def run_sync(self, prm, maxiterations, stop=None, fail_codes=()):
        """The synchronous loop on the attached handle: one ``clrsdp_iterate`` per body, the host
        decides pd_feas and terminate().  Returns why it ended: "terminated", "maxiterations",
        what ``stop(history)`` answered (asked after terminate() and the iteration bound, on the
        gaps of the states this handle's bodies produced), or "failed:<code>" when a body raised a
        ClrsdpError whose code is in ``fail_codes`` (the state is then the one before that body)."""
        dev = self.dev
        while True:
            if self.term():
                self.status = "terminated"
                return "terminated"
            if not self.it < maxiterations:
                return "maxiterations"
            why = stop(self.history) if stop is not None else None
            if why:
                return why
            if self.it == 3:
                self.t_after2 = time.time()
            try:
                st = dev.iterate(prm, self.pd_feas)
            except _lib.ClrsdpError as e:
                if e.code in fail_codes:
                    return "failed:%d" % e.code
                raise
            if self.record_exact:
                sc = dev.buffer(_lib.BUF_SCALARS, exact=True)
                self.exact.append({k: sc[v] for k, v in _lib.SC.items()})
            self.record(st)

    def result(self, return_info, stages=None):
        """The table's footer and the returned tuple (MPMP.jl:973-1024) from the attached handle."""
        dev, out, b0f = self.dev, self.out, self.b0f
        p_obj, d_obj = self.p_obj, self.d_obj
        t_total = time.time() - self.t_start
        out(HEADER)
        out(_time_spent(t_total, self.phase / 1e3 if self.timed else None,
                        self.inner / 1e3 if self.timed else None))
        xf, Xf, yf, Yf = dev.get_state()
        P, d = dev.global_P_d()
        p = dev.buffer(_lib.BUF_PVEC)
        gap_nob0 = abs((p_obj - b0f) - (d_obj - b0f)) / max(1.0, abs((p_obj - b0f) + (d_obj - b0f)))
        ret_p, ret_d = p_obj, d_obj
        if dev.w > 1:
            # MPMP.jl:1021-1023 at the state's precision: the device's objectives of the final state
            # (all limbs) and the gap without b0 from them
            import mpmath
            with mpmath.workprec(64 * dev.w + 64):
                sc = dev.buffer(_lib.BUF_SCALARS, exact=True)
                ret_p, ret_d = +sc[_lib.SC["p_obj"]], +sc[_lib.SC["d_obj"]]
                b0m = mpmath.mpf(self.b0)
                pp, dd_ = ret_p - b0m, ret_d - b0m
                gap_nob0 = abs(pp - dd_) / max(mpmath.mpf(1), abs(pp + dd_))
        res = (xf, Xf, yf, Yf, P, p, d, gap_nob0, ret_p, ret_d, t_total)
        if return_info:
            info = RunInfo(self.it - 1, self.log, self.phase, t_total,
                           (time.time() - self.t_after2) if self.t_after2 else 0.0, self.status,
                           self.exact, dev.factorization, self.lu_switch, self.inner)
            if stages is not None:
                info.stages = list(stages)
            res = res + (info,)
        return res


def _solver_params(beta_infeasible, beta_feasible, gamma, omega_p, omega_d, duality_gap_threshold,
                   primal_error_threshold, dual_error_threshold):
    kw = dict(beta_infeasible=beta_infeasible, beta_feasible=beta_feasible, gamma=gamma,
              omega_p=omega_p, omega_d=omega_d, duality_gap_threshold=duality_gap_threshold,
              primal_error_threshold=primal_error_threshold,
              dual_error_threshold=dual_error_threshold)
    return {k: (DEFAULTS[k] if v is None else v) for k, v in kw.items()}


def solverank1sdp(constraints, b, blockinfo: BlockInfo, C=None, b0=0, maxiterations=500,
                  beta_infeasible=None, beta_feasible=None, gamma=None, omega_p=None,
                  omega_d=None, duality_gap_threshold=None, primal_error_threshold=None,
                  dual_error_threshold=None, need_primal_feasible=False, need_dual_feasible=False,
                  testing=True, initial_solutions=(), precision_words=1, device=0, verbose=True,
                  solver: Optional[DeviceSolver] = None, return_info=False, record_exact=False,
                  pipelined: Optional[bool] = None, factorization: Optional[int] = None):
    """Solve the clustered low-rank SDP on the GPU; same signature/semantics as MPMP.jl:595-614.

    Returns ``(x, X, y, Y, P, p, d, duality_gap, primal_objective, dual_objective, time)``
    (MPMP.jl:1014-1024); with ``return_info`` a :class:`RunInfo` is appended.

    ``pipelined`` (default: on when the clusters are sharded over ranks): the host stays one loop body behind
    the device (clrsdp_iterate_async / _wait) and pd_feas / terminate() are evaluated on the
    device with the same thresholds, so no host round trip separates two loop bodies.  The
    iterates, the log and the returned values are the same as the synchronous loop's.

    ``factorization``: clrsdp_set_factorization flags (default FACT_FALLBACK: Cholesky, and the
    reference's pivoted LU once a Cholesky fails, announced like MPMP.jl:776-778).  At
    double-double and quad-double the returned gap and objectives are mpmath numbers at the
    state's full precision (MPMP.jl:1021-1023), not leading limbs; at fp64 they are floats.  The
    log rows (RunInfo.log) are floats except the gap column, which is an mpmath number at dd/qd
    like the returned gap (:func:`log_row`).
    """
    prm_v = _solver_params(beta_infeasible, beta_feasible, gamma, omega_p, omega_d,
                           duality_gap_threshold, primal_error_threshold, dual_error_threshold)
    out = print if verbose else (lambda *a, **k: None)
    bi = blockinfo
    dev = solver or DeviceSolver(constraints, b, bi, precision_words=precision_words, C_blocks=C,
                                 device=device)
    prm = make_params(prm_v["beta_infeasible"], prm_v["beta_feasible"], prm_v["gamma"], b0)
    loop = _Loop(prm_v, b0, need_primal_feasible, need_dual_feasible, out, testing, record_exact)
    if initial_solutions is not None and len(initial_solutions) == 4:
        x, X, y, Y = initial_solutions
    else:
        x, X, y, Y = initial_point(bi, float(prm_v["omega_p"]), float(prm_v["omega_d"]))
    dev.set_state(x, X, y, Y)
    if factorization is not None:
        dev.set_factorization(factorization)
    loop.attach(dev)
    if pipelined is None:
        # one GPU: the hipGraph replay leaves only a short host round trip between bodies and
        # the synchronous loop measured faster; sharded: enqueueing (exchange callbacks, no
        # graph) is host-heavy, so the host runs one body ahead
        pipelined = dev.world > 1 and not record_exact
    dev.set_control(make_control(prm_v["duality_gap_threshold"], prm_v["primal_error_threshold"],
                                 prm_v["dual_error_threshold"], need_primal_feasible,
                                 need_dual_feasible))
    out(HEADER)
    loop.start(dev.initial_residuals(prm))

    if pipelined:
        # the host one loop body behind: body it+1 is enqueued before the log row of body it is
        # read; the device decides pd_feas and terminate() itself (same thresholds) and a body
        # enqueued after termination applies nothing (ran = False)
        inflight = 0
        halted = False
        if loop.term():
            loop.status = "terminated"
        elif loop.it < maxiterations:
            dev.iterate_async(prm)
            inflight = 1
        try:
            while inflight:
                if loop.it + 1 < maxiterations:
                    dev.iterate_async(prm)
                    inflight += 1
                if loop.it == 3:
                    loop.t_after2 = time.time()
                st, ran = dev.iterate_wait()
                inflight -= 1
                if not ran:
                    halted = True
                    break
                loop.record(st)
        finally:
            while inflight:   # drain skipped bodies (or the one behind a failure)
                try:
                    dev.iterate_wait()
                except Exception:
                    pass
                inflight -= 1
        if loop.it > 1 or halted:
            # the reference evaluates terminate() (which prints the reason) before iter < maxit
            if loop.term() or halted:
                loop.status = "terminated"
    else:
        loop.run_sync(prm, maxiterations)
    res = loop.result(return_info)
    if solver is None:
        dev.close()
    return res


# the default hand-over floors of solve_escalating: the square root of the width's unit roundoff.
# The Newton system's conditioning grows like 1/mu, so its rounding error u/mu passes mu there;
# each sits two decades inside the recorded reach of its width (fp64: gap 1.3e-10 on the
# polynomial-minimum instance; double-double: 1e-20 on the golden instances with a
# stall near 1e-22)
GAP_FLOORS = {1: 1e-8, 2: 1e-16}


def stage_decision(history, floor, patience):
    """Whether a non-final width of :func:`solve_escalating` hands its iterate over now; a pure
    function of ``history``, the duality gaps of the states this width's loop bodies produced, in
    order (the state the width started from is not among them).  Asked after terminate() at the
    caller's thresholds.  Returns

    * ``"floor"`` when the last two gaps are both below ``floor`` (0 or None: no floor).  Two in
      a row, both produced by bodies of this width: the gap is 0 at the initial point and can
      cross zero while the iterate is still infeasible;
    * ``"stalled"`` when the last ``patience`` states set no new minimum of this width's gap (a
      width that has reached its precision wanders; its step lengths do not show it);
    * ``None`` otherwise."""
    h = list(history)
    if floor and len(h) >= 2 and h[-1] < floor and h[-2] < floor:
        return "floor"
    patience = int(patience)
    if patience > 0 and len(h) > patience and not min(h[-patience:]) < min(h[:-patience]):
        return "stalled"
    return None


def solve_escalating(constraints, b, blockinfo: BlockInfo, widths=(1, 2, 4), gap_floors=None,
                     patience=5, C=None, b0=0, maxiterations=500, beta_infeasible=None,
                     beta_feasible=None, gamma=None, omega_p=None, omega_d=None,
                     duality_gap_threshold=None, primal_error_threshold=None,
                     dual_error_threshold=None, need_primal_feasible=False,
                     need_dual_feasible=False, testing=True, initial_solutions=(),
                     precision_words=None, device=0, verbose=True, solver=None, return_info=False,
                     record_exact=False, pipelined=None, factorization: Optional[int] = None,
                     solver_factory=None):
    """One solve across word widths: :func:`solverank1sdp`'s synchronous loop, run at
    ``widths[0]`` while that is good enough and continued at the next width from the same iterate
    (``DeviceSolver.handoff_state_to``, device to device), down to the last width, whose behaviour
    is solverank1sdp's, errors included.  ``widths`` is strictly increasing, from {1, 2, 4}.

    A non-final width ends (:func:`stage_decision`, after terminate() at the caller's thresholds,
    which ends the solve at that width as today) when two states in a row have a gap below its
    floor (``gap_floors``, one per non-final width, default :data:`GAP_FLOORS`; 0: no floor), when
    ``patience`` states in a row set no new minimum of its gap, or when a loop body fails with
    E_NOT_PD_X / _S / _Q or E_STEP after the handle's own LU fallback (the device applied no
    update, so the state before that body is handed over).  An early hand-over costs only time
    and a late one only loop bodies, so no result depends on these values.

    One handle per width, created when its stage starts and closed after its hand-over; each
    uploads the constraints at its own width and gets ``factorization`` afresh (an LU fallback of
    the narrower width is not inherited).  ``maxiterations`` bounds the bodies of all widths
    together; iteration numbers and the time column continue; a line announces each switch.
    Returns the tuple of the width the solve ended at; ``RunInfo.stages`` lists
    ``(words, first iteration, bodies, reason)`` with reason one of floor, stalled,
    failed:<code>, terminated, maxiterations.

    ``precision_words``, ``solver`` and ``pipelined=True`` contradict ``widths`` and raise
    ValueError, as does a handle sharded over ranks: every rank would decide alike (the gap is
    replicated and the status words are OR-ed over the ranks), but that has not been run.
    ``solver_factory(words)`` replaces the DeviceSolver construction (tests)."""
    widths = tuple(int(w) for w in widths)
    if not widths or any(w not in (1, 2, 4) for w in widths) or \
            any(a >= c for a, c in zip(widths, widths[1:])):
        raise ValueError("widths: strictly increasing, from 1, 2, 4")
    if precision_words is not None or solver is not None or pipelined:
        raise ValueError("solve_escalating creates one synchronous handle per width: "
                         "precision_words, solver and pipelined=True do not apply")
    if gap_floors is None:
        floors = [GAP_FLOORS[w] for w in widths[:-1]]
    else:
        floors = [float(f) for f in gap_floors]
        if len(floors) != len(widths) - 1 or any(f < 0 for f in floors):
            raise ValueError("gap_floors: one value >= 0 per non-final width")
    prm_v = _solver_params(beta_infeasible, beta_feasible, gamma, omega_p, omega_d,
                           duality_gap_threshold, primal_error_threshold, dual_error_threshold)
    out = print if verbose else (lambda *a, **k: None)
    bi = blockinfo
    if solver_factory is None:
        def solver_factory(words):
            return DeviceSolver(constraints, b, bi, precision_words=words, C_blocks=C, device=device)
    prm = make_params(prm_v["beta_infeasible"], prm_v["beta_feasible"], prm_v["gamma"], b0)
    ctl = make_control(prm_v["duality_gap_threshold"], prm_v["primal_error_threshold"],
                       prm_v["dual_error_threshold"], need_primal_feasible, need_dual_feasible)
    loop = _Loop(prm_v, b0, need_primal_feasible, need_dual_feasible, out, testing, record_exact)
    stages = []
    prev = dev = None
    reason = None
    try:
        for k, w in enumerate(widths):
            dev = solver_factory(w)
            if getattr(dev, "world", 1) > 1:
                raise ValueError("solve_escalating does not run sharded over ranks")
            if prev is None:
                if initial_solutions is not None and len(initial_solutions) == 4:
                    x, X, y, Y = initial_solutions
                else:
                    x, X, y, Y = initial_point(bi, float(prm_v["omega_p"]), float(prm_v["omega_d"]))
                dev.set_state(x, X, y, Y)
            else:
                prev.handoff_state_to(dev)
                prev.close()
                prev = None
                out("Continuing at %d words from %d at iteration %d (%s)" % (
                    w, widths[k - 1], loop.it, reason))
            if factorization is not None:
                dev.set_factorization(factorization)
            loop.attach(dev)
            dev.set_control(ctl)
            if k == 0:
                out(HEADER)
            loop.start(dev.initial_residuals(prm), handed_over=k > 0)
            last = k == len(widths) - 1
            first = loop.it
            if last:
                reason = loop.run_sync(prm, maxiterations)
            else:
                floor = floors[k]
                reason = loop.run_sync(prm, maxiterations,
                                       stop=lambda h: stage_decision(h, floor, patience),
                                       fail_codes=STAGE_FAIL_CODES)
            stages.append((w, first, loop.it - first, reason))
            if reason in ("terminated", "maxiterations"):
                break
            prev, dev = dev, None
        return loop.result(return_info, stages)
    finally:
        for h in (prev, dev):
            if h is not None:
                h.close()


