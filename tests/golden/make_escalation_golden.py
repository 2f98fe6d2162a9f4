"""Generate tests/golden/rank2_mp256_seed5_gap40.json with the oracle (oracle/mpmp_oracle.py).

The 256-bit run of the ``rank2_mp256_seed5`` instance to termination at thresholds 1e-40: what a
solve that escalates fp64 -> double-double -> quad-double (solver.solve_escalating) has to arrive
at, and the number of loop bodies one width alone needs (tests/test_gpu_escalation.py).  The
format is make_golden.py's.

    python tests/golden/make_escalation_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import run  # noqa: E402

if __name__ == "__main__":
    run("rank2_mp256_seed5_gap40", dict(J=2, delta=3, rank=2, n_y=3, seed=5), 200, prec=256,
        params=dict(omega_p=10.0, omega_d=10.0, duality_gap_threshold=1e-40,
                    primal_error_threshold=1e-40, dual_error_threshold=1e-40))
