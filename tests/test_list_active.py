"""The stopping check and the list of active trajectories behind it (csrc/tog_runtime.cpp: k_batch_stats,
k_list_active and the compacted launches of tog_solve_step; DESIGN.md §5 "One preparation launch" has why the
check's commands stay as they are).

A batch of B = 600 cartpole AL problems (N = 13) of which `k` are real swing-ups and the others start converged
(the upright equilibrium, which is the goal, with zero controls): after the first steps only the k are active, the
check reports k, and every later tog_solve_step launches over a list of them. k in {0, 1, 255, 256, 257, 600}: an
empty list, one entry, one short of / exactly / one more than four full waves of entries, and the whole batch (no
list: last_active = B). The active ones sit at scattered indices, so the list's order is not the batch's prefix.

* The solve must equal TOG_NO_COMPACT=1 (launches over the whole batch, no list) bit for bit: X, U, statistics.
* Every tog_batch_stats must return the numbers of a host reduction over tog_get's statistics rows in the kernel's
  own order (lane t takes rows t, t + 1024, ...; then the halving tree over the 1,024 partials), so the comparison
  is exact.
"""
import os

import numpy as np
import pytest

B, N = 600, 13
COUNTS = [0, 1, 255, 256, 257, B]


def _problem(tog, k):
    n, m, dt = 4, 1, 0.05
    xf = np.array([0.0, np.pi, 0.0, 0.0])
    rng = np.random.default_rng(600)
    hard = np.sort(rng.permutation(B)[:k])
    x0 = np.tile(xf, (B, 1))
    U0 = np.zeros((B, N - 1, m))
    x0[hard] = 0.1 * rng.standard_normal((k, n))
    U0[hard] = 0.01 + 0.5 * rng.standard_normal((k, N - 1, m))
    cons = tog.Constraints(N)
    bnd = tog.BoundConstraint(n, m, u_min=-3.0, u_max=3.0)
    for i in range(N - 1):
        cons[i] += bnd
    cons[N - 1] += tog.goal_constraint(xf)
    obj = tog.LQRObjective(1e-2 * np.eye(n), 1e-1 * np.eye(m), 100.0 * np.eye(n), xf, N)
    prob = tog.Problem(tog.rk3(tog.Dynamics.cartpole), obj, U0, x0=x0, xf=xf, N=N, dt=dt, constraints=cons)
    il = tog.iLQRSolverOptions(iterations=12)
    return prob, tog.AugmentedLagrangianSolverOptions(opts_uncon=il, iterations=3), hard


def _host_stats(S, A):
    """k_batch_stats' reduction on the host, in its order."""
    act = np.zeros(1024)
    J = np.zeros(1024)
    c = np.zeros(1024)
    for t in range(min(1024, S.shape[0])):
        rows = S[t::1024]
        for r in rows:
            act[t] += 1.0 if int(r[A.STAT_FLAGS]) & A.TRAJ_ACTIVE else 0.0
            J[t] += r[A.STAT_J]
            c[t] = max(c[t], r[A.STAT_C_MAX])
    w = 512
    while w > 0:
        act[:w] += act[w:2 * w]
        J[:w] += J[w:2 * w]
        c[:w] = np.maximum(c[:w], c[w:2 * w])
        w //= 2
    return np.array([act[0], J[0], c[0]])


def _run(tog, k, env):
    A = tog.abi
    old = {e: os.environ.get(e) for e in env}
    for e, v in env.items():
        if v is None:
            os.environ.pop(e, None)
        else:
            os.environ[e] = v
    try:
        prob, opts, hard = _problem(tog, k)
        h = tog.AbstractSolverFor(prob, opts).handle
        h.solve_init(A.MODE_AL)
        checks = []
        for _ in range(8):  # the converged starts finish within their first steps; the swing-ups do not
            h.solve_step(1)
            S = h.get(A.FIELD_STATS)
            active = np.flatnonzero(S[:, A.STAT_FLAGS].astype(np.int64) & A.TRAJ_ACTIVE)
            if len(active) == k:
                break
        assert np.array_equal(active, hard), "the batch did not come down to the k swing-ups"
        for _ in range(12):
            st = h.batch_stats()  # the stopping check: the next steps launch over ceil(st[0]) slots
            S = h.get(A.FIELD_STATS)
            assert not np.isnan(S[:, [A.STAT_J, A.STAT_C_MAX]]).any()
            assert np.array_equal(st, _host_stats(S, A)), (st, _host_stats(S, A))
            checks.append(st)
            if st[0] == 0.0:
                break
            h.solve_step(4)
        return h.get(A.FIELD_X), h.get(A.FIELD_U), h.get(A.FIELD_STATS), np.array(checks)
    finally:
        for e, v in old.items():
            if v is None:
                os.environ.pop(e, None)
            else:
                os.environ[e] = v


@pytest.mark.gpu
@pytest.mark.parametrize("k", COUNTS)
def test_listed_steps_equal_whole_batch_steps(tog, gpu, k):
    a = _run(tog, k, {"TOG_NO_COMPACT": None})
    b = _run(tog, k, {"TOG_NO_COMPACT": "1"})
    assert a[3][0][0] == k  # the first check saw exactly the k swing-ups
    if k:
        assert a[2][:, tog.abi.STAT_TOTAL_STEPS].max() > 8  # steps ran behind a check, over the list
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
