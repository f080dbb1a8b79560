"""Projected Newton's wide path (blocks of 65-128 rows, tog_pn.hpp T = 128), timed.

    python tools/pn_wide_bench.py [--batch 256] [--ft 1e-10] [--out file.json]

The problem of tests/test_pn_wide.py (the car with 64 coincident circles: 72 rows a stage knot, blocks of 68-69
rows at 4-6 knots after the AL phase), its three AL iterates from the CPU oracle tiled to the batch. One
tog_solve_pn (:feasible, three newton steps): every trajectory overflows the narrow pass and is solved again by
the wide kernels, so the time covers both passes. A capability path: the figure is a baseline, not a target."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ft", type=float, default=1e-10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tog = __graft_entry__.load_package()
    oracle = __graft_entry__.load_oracle()
    import test_pn_wide as W
    W.al_start(tog, oracle, "wide")
    opts = W.pn_opts(tog, a.ft)
    W.device_pn(tog, W.pick(tog, W.WIDE3), opts)  # warm-up: module loading, first-launch costs
    prob = W.pick(tog, [("wide", b % 3) for b in range(a.batch)])
    solver = tog.ProjectedNewtonSolver(prob, opts)
    solver.handle.upload_state(prob)
    t0 = time.perf_counter()
    out = solver.handle.solve_pn(tog.to_tog_pn_options(opts))
    dt = time.perf_counter() - t0
    flags = np.asarray(solver.handle.status())
    out = np.asarray(out)
    lib = tog.abi.load_library()
    with open(lib._name, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()[:16]
    c_max = out[:, tog.abi.PN_C_MAX]
    line = {
        "what": "projected Newton, wide path: car with 64 coincident circles (72 rows a knot), :feasible, 3 steps",
        "libtog_sha16": sha, "batch": a.batch, "feasibility_tolerance": a.ft,
        "time_pn_s": round(dt, 4), "per_trajectory_ms": round(1e3 * dt / a.batch, 4),
        "c_max_max": float(np.max(c_max)),
        "pn_error": int(np.count_nonzero(flags & tog.abi.TRAJ_PN_ERROR)),
        "pn_block": int(np.count_nonzero(flags & tog.abi.TRAJ_PN_BLOCK)),
    }
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
