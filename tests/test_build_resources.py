"""The compiler's resource report of the in-tree library (clustered-low-rank-sdp-solver_amd/build.py
writes it beside libclrsdp.so on every build): no kernel of the benchmarked paths spills
registers to scratch memory.  A spill is a silent slowdown the parity tests cannot see -- round 6
found schur_fused_f64 at 92 B/lane (C3 Schur launch 57 -> 64 us) after a runtime branch was added
to its epilogue."""
import os
import subprocess

import pytest

import _clrsdp_pkg

# known spills, off every benchmarked configuration (C1-C5):
ALLOWED = (
    "getrf_batched<",   # the pivoted-LU fallback (approx_lu!), taken only when Cholesky fails
    "potrf_batched<",   # the panel potrf beyond chol_lookahead's sizes (dd > 128 with CLRSDP_POTRF_BLK=0, qd > 64)
    # quad-double X / Y blocks of 33..64 with L^-1 at 1024 threads (128 VGPRs per lane); C5's
    # X / Y blocks are <= 18 and take the 256-thread instance, which does not spill
    "chol_lookahead<mw::qd, true,",
)


def _demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    out = r.stdout.splitlines() if r.returncode == 0 else []
    return out if len(out) == len(names) else list(names)


def test_no_kernel_spills_to_scratch():
    b = _clrsdp_pkg.load_build()
    if not os.path.exists(b.RESOURCES):
        pytest.skip("library built without the resource report (run __graft_entry__.build())")
    res = b.kernel_resources()
    assert len(res) > 50, len(res)
    spilling = [k for k, v in res.items() if v.get("ScratchSize", 0) > 0]
    bad = {d: res[k]["ScratchSize"] for k, d in zip(spilling, _demangle(spilling))
           if not any(a in d for a in ALLOWED)}
    assert not bad, bad
