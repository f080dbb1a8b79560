#!/usr/bin/env python3
"""Sequential batches against one streamed solve, config 3 (quadrotor AL-iLQR, square-root backward pass).

Three start sets, ``config_quadrotor(B, offset)`` at offsets 0, B and 2B (B = 8192 by default):

  (a) three ``tog_solve``s one after the other on one handle of B trajectories;
  (b) one ``tog_solve_stream`` of the 3B jobs through a handle of B slots.

Reports the total iLQR iterations, seconds and iterations/s of both, whether every job's X and U are bitwise
equal between the two, and the cost of a refill: HIP events (torch.cuda.Event on the handle's stream) around one
``tog_refill`` call of 1, 64 and 1,024 listed slots. Such a call is the state check's gather and its copy back, the
host's staging, the host -> device copies of x0 and U, k_refill and the slot marks; the events therefore bound
k_refill from above. Writes one JSON object (``--out``, default profiles/stream_bench.json).

    python tools/stream_bench.py [--B 8192] [--sets 3] [--out profiles/stream_bench.json]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import __graft_entry__  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stream_bench.json"))
    a = ap.parse_args()
    tog = __graft_entry__.load_package()
    A = tog.abi
    import torch

    B, K = a.B, a.sets
    sets = [tog.Problems.config_quadrotor(B=B, offset=k * B) for k in range(K)]
    opts = sets[0][1]
    mode = A.MODE_AL

    # (a) sequential: one handle, one tog_solve per set
    solver = tog.AbstractSolverFor(sets[0][0].copy(), opts, device=0)
    h = solver.handle
    warm = sets[0][0].copy()
    h.upload_state(warm)
    h.solve(mode, max_steps=8)  # (first launches: code object load)
    h.synchronize()
    seq = {"sets": [], "iterations": 0, "seconds": 0.0}
    Xa, Ua = [], []
    for k, (prob, _) in enumerate(sets):
        p = prob.copy()
        h.upload_state(p)
        h.synchronize()
        t0 = time.perf_counter()
        h.solve(mode)
        h.synchronize()
        dt = time.perf_counter() - t0
        h.download_state(p)
        S = h.get(A.FIELD_STATS)
        it = int(S[:, A.STAT_TOTAL_STEPS].sum())
        seq["sets"].append({"offset": k * B, "iterations": it, "seconds": round(dt, 4),
                            "max_traj_iterations": int(S[:, A.STAT_TOTAL_STEPS].max())})
        seq["iterations"] += it
        seq["seconds"] += dt
        Xa.append(p._X)
        Ua.append(p._U)
    seq["seconds"] = round(seq["seconds"], 4)
    seq["rate"] = round(seq["iterations"] / seq["seconds"], 2)
    Xa, Ua = np.concatenate(Xa), np.concatenate(Ua)

    # (b) streamed: the K x B jobs through B slots of the same handle
    x0 = np.concatenate([p.x0 for p, _ in sets])
    U0 = np.concatenate([p._U for p, _ in sets])
    h.solve_stream(mode, x0[:2], U0[:2], max_steps=4)  # (first use: the staging buffers are allocated here)
    h.synchronize()
    t0 = time.perf_counter()
    Xb, Ub, Sb, done = h.solve_stream(mode, x0, U0)
    h.synchronize()
    dt = time.perf_counter() - t0
    it = int(Sb[:, A.STAT_TOTAL_STEPS].sum())
    stream = {"jobs": int(K * B), "slots": B, "jobs_done": done, "iterations": it, "seconds": round(dt, 4),
              "rate": round(it / dt, 2), "max_traj_iterations": int(Sb[:, A.STAT_TOTAL_STEPS].max())}
    same = bool(np.array_equal(Xa, Xb) and np.array_equal(Ua, Ub))
    del solver, h

    # the cost of a refill, from HIP events on the handle's stream
    st = torch.cuda.Stream()
    rs = tog.AbstractSolverFor(sets[0][0].copy(), opts, device=0, stream=st.cuda_stream)
    rh = rs.handle
    rh.solve_init(mode)
    rh.solve_step(1)
    rh.synchronize()
    # every slot inactive: a streamed solve of no jobs clears the slots and starts nothing
    rh.solve_stream(mode, x0[:0], U0[:0])
    refill = []
    for count in (1, 64, 1024):
        if count > B:
            continue
        slots = np.arange(count, dtype=np.int32)
        us = []
        for rep in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                rh.refill(slots, x0[:count], U0[:count])
                e1.record(st)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
            rh.solve_stream(mode, x0[:0], U0[:0])  # the slots inactive again for the next repetition
        refill.append({"slots": count, "us_per_call_median": round(float(np.median(us[1:])), 1),
                       "us_per_call_min": round(float(np.min(us[1:])), 1)})
    out = {"config": "config_quadrotor (config 3), AL-iLQR, square-root backward pass", "B": B, "sets": K,
           "sequential": seq, "streamed": stream, "speedup": round(seq["seconds"] / stream["seconds"], 3),
           "bitwise_equal_X_U": same,
           "refill_call_us": refill,
           "refill_note": "HIP events around one tog_refill call: state-check gather and copy back, host staging, "
                          "host->device copies of x0 and U, k_refill, slot marks (an upper bound of k_refill)"}
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
