"""The build's resource report (clustered-low-rank-sdp-solver_amd/build.py writes it beside
libclrsdp.so) lists the fp64 and quad-double instances of the blocked Cholesky chain that
CLRSDP_POTRF_BLK=1 selects (MatPlan::potrf), and none of them uses scratch memory (a
conditional expression on a whole quad-double left a 32-byte stack slot in the staging loops of
potrf_blk_trsm / potrf_blk_update; test_build_resources.py has no allowance for these kernels)."""
import os

import pytest

import _clrsdp_pkg
from test_build_resources import _demangle

CHAIN = (
    "potrf64_first<16>", "potrf64_trsm<16>", "potrf64_update<16>",
    "potrf_blk_first<mw::qd, true, 16>", "potrf_blk_trsm<mw::qd, 16>",
    "potrf_blk_update<mw::qd, true, 16>",
)


def test_chain_instances_are_built_without_scratch():
    b = _clrsdp_pkg.load_build()
    if not os.path.exists(b.RESOURCES):
        pytest.skip("library built without the resource report (run __graft_entry__.build())")
    res = b.kernel_resources()
    names = list(res)
    by_name = dict(zip(_demangle(names), names))
    for k in CHAIN:
        hits = [d for d in by_name if f"clrsdp::{k}(" in d.replace("void ", "")]
        assert len(hits) == 1, (k, hits)
        r = res[by_name[hits[0]]]
        print(hits[0], r)
        assert r["ScratchSize"] == 0, (hits[0], r)
