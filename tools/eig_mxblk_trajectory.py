"""Flagged share of the mxblk route on a trajectory: one double-double solve
of the step_timing instance (J = 2, n_y = 8, X/Y blocks of D and 12) with CLRSDP_EIG_MX_BLK=1,
stopped after K loop bodies for each K given, from the same initial point (Omega = 10).  A
solve that ends in a solver error is reported with the error as its status.  With
CLRSDP_EIGMX_STATS=1 the library prints its process-wide count of flagged blocks (n >= 3) when a
handle is destroyed; the count of each solve is the difference to the line before it, read here
from the process's own stderr.  Every body runs lambda_min on four blocks (X and Y, D and 12).
One JSON line per K.  From the repository root:
    python tools/eig_mxblk_trajectory.py D K1 K2 ...      (e.g. 100 5 20 200)
"""
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
os.environ["CLRSDP_EIG_MX_BLK"] = "1"
os.environ["CLRSDP_EIGMX_STATS"] = "1"
import _clrsdp_pkg  # noqa: E402

pk = _clrsdp_pkg.load()
from helpers import _sp  # noqa: E402

D = int(sys.argv[1])
cons, b = pk.synth_mixed([_sp(1, [D], 32), _sp(1, [12], 32)], 8, seed=7)
bi = pk.get_block_info(cons)
assert pk.eigmin_kernel(D, 2) == 6
err = tempfile.TemporaryFile(mode="w+")
saved = os.dup(2)
os.dup2(err.fileno(), 2)
rows = []
try:
    for K in (int(v) for v in sys.argv[2:]):
        dev = pk.DeviceSolver(cons, b, bi, precision_words=2)
        try:
            out = pk.solverank1sdp(cons, b, bi, maxiterations=K, omega_p=10, omega_d=10,
                                   precision_words=2, solver=dev, verbose=False, return_info=True)
            rows.append((K, out[-1].iterations, out[-1].status, float(out[7])))
        except Exception as e:  # noqa: BLE001
            rows.append((K, None, f"error: {e}", None))
        finally:
            dev.close()
finally:
    os.dup2(saved, 2)
err.seek(0)
counts = [int(v) for v in re.findall(r"fallbacks so far: (\d+)", err.read())]
prev = 0
for (K, its, status, gap), c in zip(rows, counts):
    print(json.dumps({"tool": "eig_mxblk_trajectory", "words": 2, "delta": D, "maxiterations": K,
                      "bodies": its, "status": status, "duality_gap": gap, "flagged_blocks": c - prev,
                      "blocks_per_body": 4}), flush=True)
    prev = c
