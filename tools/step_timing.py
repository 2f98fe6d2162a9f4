"""STEP stage time with CLRSDP_EIG_BLK on against unset: per-stage HIP
events (set_timing(1), no graph), median of 10 loop bodies restarted from the initial point
Omega = 10, on a handle with J = 2, n_y = 8 and X/Y blocks of D and 12; each setting twice,
alternating, on a fresh handle (the switch is read when the handle's plans are finalised).  One
JSON line per handle.  From the repository root:
    python tools/step_timing.py WORDS D [SWITCH] (e.g. 1 640, 4 160; 4 160 CLRSDP_EIG_MX_BLK)
SWITCH names the environment switch that is alternated (default CLRSDP_EIG_BLK).
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import _clrsdp_pkg  # noqa: E402

pk = _clrsdp_pkg.load()
from clrsdp_amd import _lib as L  # noqa: E402
from oracle import mpmp_oracle as oracle  # noqa: E402
from helpers import _sp  # noqa: E402

words, D = int(sys.argv[1]), int(sys.argv[2])
SWITCH = sys.argv[3] if len(sys.argv) > 3 else "CLRSDP_EIG_BLK"
cons, b = pk.synth_mixed([_sp(1, [D], 32), _sp(1, [12], 32)], 8, seed=7)
bi = oracle.get_block_info(cons)
ar = oracle.Fp64()
state = oracle.initial_point(ar, bi, 10.0, 10.0)
P = pk.make_params("0.3", "0.1", "0.7", 0)
for sw in (None, "1", None, "1"):
    if sw is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = sw
    kern = pk.eigmin_kernel(D, words)
    dev = pk.DeviceSolver(cons, b, pk.get_block_info(cons), precision_words=words)
    try:
        dev.set_state(*state)
        dev.save_state()
        dev.set_timing(1)
        step, body, lam = [], [], None
        for it in range(11):
            dev.restore_state()
            st = dev.iterate(P, False)
            if it:
                step.append(st.phase_ms[L.STAGE_STEP])
                body.append(sum(st.phase_ms[:]))
        lam = float(dev.scalar("mineig_X"))
    finally:
        dev.close()
    print(json.dumps({"tool": "step_timing", "words": words, "delta": D, SWITCH: sw,
                      "eig_kernel": L.EIG_K_NAMES[kern], "step_stage_ms_median": float(np.median(step)),
                      "step_stage_ms_min": float(np.min(step)), "body_ms_median": float(np.median(body)),
                      "mineig_X": lam}), flush=True)
