#!/usr/bin/env python3
"""Cost of per-trajectory bounds on config 3's all-active window: the bench's 20-step window (tog_solve_init,
5 warm-up steps, 20 timed steps of one batch step each) with config_quadrotor_bounds(B) against the shared
bounds of config_quadrotor(B) on the same build, a few repetitions each, interleaved. Prints one JSON line.

    python tools/traj_bounds_cost.py [--batch 8192] [--steps 20] [--warmup 5] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import __graft_entry__  # noqa: E402


def window_ms(h, mode, warmup, steps):
    h.solve_init(mode)
    h.solve_step(warmup)
    h.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        h.solve_step(1)
    h.synchronize()
    t1 = time.perf_counter()
    n_active = h.batch_stats()[0]
    return 1e3 * (t1 - t0) / steps, n_active


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    out = {"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "reps": a.reps}
    solvers = {}
    for name, make in (("shared", pkg.Problems.config_quadrotor), ("bounds", pkg.Problems.config_quadrotor_bounds)):
        prob, opts = make(B=a.batch)
        solvers[name] = (pkg.AugmentedLagrangianSolver(prob, opts), prob)
    ms = {k: [] for k in solvers}
    act = {k: [] for k in solvers}
    for _ in range(a.reps):
        for name, (s, prob) in solvers.items():
            s.handle.upload_state(prob)
            t, n = window_ms(s.handle, s.mode, a.warmup, a.steps)
            ms[name].append(round(t, 4))
            act[name].append(int(n))
    for name in solvers:
        out[name] = {"ms_per_step": ms[name], "median": statistics.median(ms[name]), "min": min(ms[name]),
                     "max": max(ms[name]), "n_active_after": act[name]}
    out["bounds_over_shared"] = round(out["bounds"]["median"] / out["shared"]["median"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
