#!/usr/bin/env python3
"""Cost of per-trajectory cost weights on config 3, two figures on one build:

window: the bench's 20-step all-active window (tog_solve_init, 5 warm-up steps, 20 timed steps of one batch step
each) with config_quadrotor_weights(B) against the shared weights of config_quadrotor(B), a few repetitions each,
interleaved;

tail: a single trajectory solved alone (tools/tail_solve.py's loop: solve_step(chunk) and the blocking batch_stats
readback until nothing is active), where the Hessian reads sit on the backward pass's serial chain: member `offset`
of config_quadrotor_weights as a B = 1 weights handle against the same member as a plain problem that carries its
Hessians in the descriptor (Problem.trajectory). Both solve the same problem bit for bit, so the step counts agree
and the ratio of ms per batch step is the table's cost.

Prints one JSON line.

    python tools/traj_weights_cost.py [--batch 8192] [--steps 20] [--warmup 5] [--reps 5] [--offset 7] [--chunk 4]
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


def tail_ms(h, mode, chunk):
    h.synchronize()
    t0 = time.perf_counter()
    h.solve_init(mode)
    done = 0
    while done < 20000:
        h.solve_step(chunk)
        done += chunk
        if h.batch_stats()[0] == 0.0:
            break
    h.synchronize()
    return 1e3 * (time.perf_counter() - t0) / done, done, h.total_steps()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--offset", type=int, default=7, help="the member solved alone for the tail figure")
    ap.add_argument("--chunk", type=int, default=4)
    a = ap.parse_args()
    pkg = __graft_entry__.load_package()
    out = {"batch": a.batch, "steps": a.steps, "warmup": a.warmup, "reps": a.reps}
    solvers = {}
    for name, make in (("shared", pkg.Problems.config_quadrotor), ("weights", pkg.Problems.config_quadrotor_weights)):
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
    out["weights_over_shared"] = round(out["weights"]["median"] / out["shared"]["median"], 4)
    del solvers

    # the single-trajectory tail: the same member with the table, and with its Hessians in the descriptor
    batch, opts = pkg.Problems.config_quadrotor_weights(B=a.offset + 1)
    table = batch.batch_slice(a.offset, a.offset + 1)
    plain = batch.trajectory(a.offset)
    assert table.has_trajectory_weights() and not plain.has_trajectory_data()
    tail = {"offset": a.offset, "chunk": a.chunk}
    pairs = {"descriptor": plain, "table": table}
    hs = {k: pkg.AugmentedLagrangianSolver(p, opts) for k, p in pairs.items()}
    res = {k: [] for k in pairs}
    for rep in range(a.reps + 1):  # (the first repetition warms the code objects and is dropped)
        for k, s in hs.items():
            s.handle.upload_state(pairs[k])
            t, done, iters = tail_ms(s.handle, s.mode, a.chunk)
            if rep:
                res[k].append(round(t, 5))
            tail[k + "_batch_steps"], tail[k + "_iterations"] = done, iters
    for k in pairs:
        tail[k] = {"ms_per_batch_step": res[k], "median": statistics.median(res[k])}
    tail["table_over_descriptor"] = round(tail["table"]["median"] / tail["descriptor"]["median"], 4)
    out["tail"] = tail
    print(json.dumps(out))


if __name__ == "__main__":
    main()
