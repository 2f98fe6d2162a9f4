"""The build's resource report (clustered-low-rank-sdp-solver_amd/build.py writes it beside
libclrsdp.so) lists every instance of the eigblk_* chain that MatPlan::eigmin can launch with
CLRSDP_EIG_BLK=1 -- the two prepass kernels and the column kernel at the plan's strip height
(MatPlan::EIG_R = 64), eigblk_sturm with the tridiagonal in LDS and in global memory -- at each
word width, once, and none of them uses scratch memory (multi-word selects go limb by limb;
test_build_resources.py has no allowance for these kernels)."""
import os

import pytest

import _clrsdp_pkg
from test_build_resources import _demangle

WORDS = ("double", "mw::dd", "mw::qd")
CHAIN = tuple(k.format(w) for w in WORDS for k in
              ("eigblk_amax<{}, 64>", "eigblk_sym<{}, 64>", "eigblk_col<{}, 64>",
               "eigblk_sturm<{}, true>", "eigblk_sturm<{}, false>"))


def test_chain_instances_are_built_without_scratch():
    b = _clrsdp_pkg.load_build()
    if not os.path.exists(b.RESOURCES):
        pytest.skip("library built without the resource report (run __graft_entry__.build())")
    res = b.kernel_resources()
    names = list(res)
    by_name = dict(zip(_demangle(names), names))
    built = [d for d in by_name if "clrsdp::eigblk_" in d]
    assert len(built) == len(CHAIN), built   # nothing but what the plan launches
    for k in CHAIN:
        hits = [d for d in by_name if f"clrsdp::{k}(" in d.replace("void ", "")]
        assert len(hits) == 1, (k, hits)
        r = res[by_name[hits[0]]]
        print(hits[0], r)
        assert r["ScratchSize"] == 0, (hits[0], r)
