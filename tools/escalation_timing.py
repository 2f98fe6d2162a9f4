"""One solve across widths against the wide width alone ("Escalating the
precision within one solve"): C4 = synth(J=16, delta=64, rank=2, n_y=64, seed=0), Omega = 10,
all thresholds 1e-20; ``solve_escalating(widths=(1, 2))`` and ``solverank1sdp(precision_words=2)``,
three repetitions, alternating.  Reports the wall time of each solve (handle construction and
constraint upload included on both sides), the loop bodies per width, and the set-up time of the
second handle on its own (its construction, plans and upload, taken inside the solve).  One JSON
line per solve, appended to profiles/escalation_timing.jsonl.  A record, not a pass mark.  From
the repository root:
    python tools/escalation_timing.py [REPETITIONS]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import _clrsdp_pkg  # noqa: E402

pk = _clrsdp_pkg.load()

SHAPE = dict(J=16, delta=64, rank=2, n_y=64, seed=0)
PARAMS = dict(omega_p=10.0, omega_d=10.0, duality_gap_threshold=1e-20, primal_error_threshold=1e-20,
              dual_error_threshold=1e-20)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
cons, b = pk.synth(**SHAPE)
bi = pk.get_block_info(cons)
out = os.path.join("profiles", "escalation_timing.jsonl")


def escalating():
    setup = {}

    def factory(words):
        t = time.time()
        dev = pk.DeviceSolver(cons, b, bi, precision_words=words)
        dev.synchronize()
        setup[words] = time.time() - t
        return dev
    t = time.time()
    res = pk.solve_escalating(cons, b, bi, widths=(1, 2), maxiterations=300, verbose=False,
                              return_info=True, solver_factory=factory, **PARAMS)
    wall = time.time() - t
    info = res[-1]
    return dict(run="escalating (1, 2)", wall_s=wall, status=info.status, iterations=info.iterations,
                stages=[list(s) for s in info.stages], bodies={str(s[0]): s[2] for s in info.stages},
                setup_s={str(k): v for k, v in setup.items()}, loop_s=info.time_total,
                gap=float(res[7]), p_obj=float(res[8]), d_obj=float(res[9]))


def plain():
    t = time.time()
    res = pk.solverank1sdp(cons, b, bi, precision_words=2, maxiterations=300, verbose=False,
                           return_info=True, **PARAMS)
    wall = time.time() - t
    info = res[-1]
    return dict(run="precision_words=2", wall_s=wall, status=info.status, iterations=info.iterations,
                bodies={"2": info.iterations}, loop_s=info.time_total, gap=float(res[7]),
                p_obj=float(res[8]), d_obj=float(res[9]))


for rep in range(reps):
    for fn in (escalating, plain):
        rec = dict(tool="escalation_timing", shape=SHAPE, thresholds=1e-20, rep=rep, **fn())
        line = json.dumps(rec)
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")
