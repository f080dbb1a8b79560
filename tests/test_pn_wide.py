"""Projected Newton blocks beyond 64 rows: the wide kernels (tog_pn.hpp, T = 128) and tog_solve_pn's second pass.

The narrow kernels give a block (n + the rows active at a knot) a row per lane of one wave. A trajectory whose
active set outgrows 64 rows used to stop with TRAJ_PN_ERROR | TRAJ_PN_BLOCK; tog_solve_pn now solves it again
from the call's starting point with the wide kernels, and leaves every other trajectory of the batch as the
narrow pass left it.

The problem is Problems.car_obstacles without obstacle2 and with obstacle1 as 64 coincident circles: a stage
knot carries 8 bound rows + 64 circle rows = 72 (PCAP), n = 3, N = 51. Coincident rows are exactly consistent,
so the :feasible projection converges while the blocks are wide (68-69 rows at 4-6 adjacent knots after the AL
phase: wide-to-wide and wide-to-narrow off-diagonal blocks both occur). Y Yᵀ of coincident rows is singular, so
:optimal raises the reference's exception on both sides: that case is parity only.

The GPU tests hold the device to the oracle (oracle/tog_oracle_pn.c, stride n + pmax, no block limit) from the
oracle's AL iterates by test_projected_newton._pn_compare's rules: X, U, cost and viol within TOL_STEP = 1e-13,
equal projections, line searches, refinements and steps, c_max within 1e-13.
"""
import math

import numpy as np
import pytest

import test_projected_newton as T

TOL_STEP = T.TOL_STEP
N, NX, NU = 51, 3, 2
X0_NARROW = np.array([-0.4, 0.0, 0.0])  # passes left of the obstacle: blocks of at most 4 rows


def wide_starts():
    """U0 = ones, then two draws of ones + 0.05 N(0, 1) from default_rng(3)."""
    rng = np.random.default_rng(3)
    U0 = np.ones((3, N - 1, NU))
    U0[1:] += 0.05 * rng.standard_normal((2, N - 1, NU))
    return U0


def wide_problem(tog, U0, x0):
    """Problems.car_obstacles (test/projected_newton_test.jl:1-27) with obstacle2 dropped and obstacle1 as 64
    coincident circles; U0 (B, N-1, m), x0 (B, n)."""
    model_d = tog.rk4(tog.Dynamics.car)
    n, m = NX, NU
    dt = 3.0 / (N - 1)
    Q, R, Qf = 0.01 * np.eye(n), 0.01 * np.eye(m), 0.01 * np.eye(n)
    xf = np.array([0.0, 1.0, 0.0])
    obj = tog.LQRObjective(Q, R, Qf, xf, N)
    bnd = tog.BoundConstraint(n, m, x_min=[-0.5, -0.01, -math.inf], x_max=[0.5, 1.01, math.inf], u_min=[0.1, -2.0],
                              u_max=1.5)
    bnd1 = tog.BoundConstraint(n, m, u_min=[0.1, -2.0])
    obs1 = tog.CircleConstraints(n, m, [[0.2, 0.6, 0.25]] * 64, label="obstacle1")
    cons = tog.Constraints(N)
    cons[0] += bnd1
    for k in range(1, N - 1):
        cons[k] += bnd
        cons[k] += obs1
    cons[N - 1] += tog.goal_constraint(xf)
    U0 = np.asarray(U0, dtype=np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    if U0.shape[0] == 1:
        U0, x0 = U0[0], x0[0]
    return tog.Problem(model_d, obj, U0, constraints=cons, x0=x0, xf=xf, N=N, dt=dt)


def pn_opts(tog, ft=1e-6, solve_type="feasible", n_steps=3):
    return tog.ProjectedNewtonSolverOptions(feasibility_tolerance=ft, active_set_tolerance=1e-4, n_steps=n_steps,
                                            solve_type=solve_type)


_CACHE = {}


def al_start(tog, oracle, kind):
    """The oracle's AL iterates (car_al_opts(tol=1e-3)), computed once: 'wide' the three x0 = 0 starts, 'narrow'
    the first two controls from x0 = [-0.4, 0, 0]."""
    if kind not in _CACHE:
        U0 = wide_starts()
        if kind == "wide":
            prob = wide_problem(tog, U0, np.zeros((3, NX)))
        else:
            prob = wide_problem(tog, U0[:2], np.tile(X0_NARROW, (2, 1)))
        _CACHE[kind] = T.oracle_al_state(tog, oracle, prob, T.car_al_opts(tog, tol=1e-3))
    return _CACHE[kind]


def pick(tog, parts):
    """A batch of AL iterates: parts = [(kind, index), ...]."""
    srcs = {k: _CACHE[k] for k, _ in parts}
    prob = wide_problem(tog, np.stack([srcs[k]._U[i] for k, i in parts]),
                        np.stack([np.atleast_2d(srcs[k].x0)[i] for k, i in parts]))
    for b, (k, i) in enumerate(parts):
        prob._X[b] = srcs[k]._X[i]
        prob._U[b] = srcs[k]._U[i]
    return prob


def oracle_pn(tog, oracle, kind, i, opts):
    """The oracle's projected Newton from AL iterate (kind, i), once per options: (X, U, statistics row, flags)."""
    key = (kind, i, opts.feasibility_tolerance, opts.solve_type, opts.n_steps)
    if key not in _CACHE:
        start = al_start(tog, oracle, kind)
        o = oracle.OracleSolver(start, T.car_al_opts(tog, tol=1e-3), b=i)
        out = o.solve_pn(opts)
        _CACHE[key] = (o.get("X"), o.get("U"), np.array(out), int(o.get("stats")[tog.abi.STAT_FLAGS]))
    return _CACHE[key]


def device_pn(tog, prob, opts):
    """Device projected Newton on prob's X, U; the reference's exception, raised after the batch, is kept aside."""
    gp = prob.copy()
    solver = tog.ProjectedNewtonSolver(gp, opts)
    try:
        tog.solve_b(gp, solver)
        raised = None
    except tog.ProjectedNewtonError as e:
        raised = e
    return gp, solver.stats, raised


def compare(tog, oracle, parts, opts):
    """_pn_compare's rules for the batch `parts`, trajectory by trajectory; returns the device's results."""
    for k in {k for k, _ in parts}:
        al_start(tog, oracle, k)
    gp, st, raised = device_pn(tog, pick(tog, parts), opts)
    abi = tog.abi
    for b, (k, i) in enumerate(parts):
        X, U, out, fo = oracle_pn(tog, oracle, k, i, opts)
        print(f"traj {b} ({k} {i}): errX {T.rel(gp._X[b], X):.2e} errU {T.rel(gp._U[b], U):.2e} flags {int(st['flags'][b]):#x} "
              f"(oracle {fo:#x}) c_max {st['c_max'][b]:.3e} (oracle {out[abi.PN_C_MAX]:.3e}) proj {st['projections'][b]} "
              f"ls {st['linesearches'][b]} ref {st['refinements'][b]} steps {st['iterations'][b]}")
    for b, (k, i) in enumerate(parts):
        X, U, out, fo = oracle_pn(tog, oracle, k, i, opts)
        assert not st["flags"][b] & abi.TRAJ_PN_BLOCK, b
        assert T.rel(gp._X[b], X) < TOL_STEP and T.rel(gp._U[b], U) < TOL_STEP, b
        for key, idx in (("projections", abi.PN_PROJECTIONS), ("linesearches", abi.PN_LINESEARCHES),
                         ("refinements", abi.PN_REFINEMENTS), ("iterations", abi.PN_STEPS)):
            assert st[key][b] == out[idx], (b, key, st[key][b], out[idx])
        assert abs(st["c_max"][b] - out[abi.PN_C_MAX]) <= 1e-13 * max(1.0, abs(out[abi.PN_C_MAX]))
        assert T.rel(st["cost"][b], out[abi.PN_J]) < TOL_STEP
        assert T.rel(st["viol"][b], out[abi.PN_VIOL]) < TOL_STEP
        assert bool(st["flags"][b] & abi.TRAJ_PN_ERROR) == bool(fo & abi.TRAJ_PN_ERROR), b
    return gp, st, raised


WIDE3 = [("wide", 0), ("wide", 1), ("wide", 2)]


# ----------------------------------------------------------------------------- CPU: the inputs


def test_wide_inputs_on_the_oracle(tog, oracle):
    """Guards the fixture: at the AL iterate of each of the three starts, 3 + #{rows of C >= -1e-4} exceeds 64 at
    3 knots or more, and the oracle's :feasible projection (which has no block limit) ends unflagged with
    c_max < 1e-6."""
    start = al_start(tog, oracle, "wide")
    for b in range(3):
        o = oracle.OracleSolver(start, T.car_al_opts(tog, tol=1e-3), b=b)
        o.update_constraints()
        assert o.pmax == 72
        C = o.get("C")[1:N - 1]  # the stage knots: 72 inequality rows each
        blocks = NX + np.sum(C >= -1e-4, axis=1)
        assert np.sum(blocks > 64) >= 3, (b, blocks.max())
        assert blocks.max() <= 128
        X, U, out, flags = oracle_pn(tog, oracle, "wide", b, pn_opts(tog, 1e-6))
        assert not flags & tog.abi.TRAJ_PN_ERROR, b
        assert out[tog.abi.PN_C_MAX] < 1e-6, (b, out[tog.abi.PN_C_MAX])


# ----------------------------------------------------------------------------- GPU: device vs oracle


@pytest.mark.gpu
@pytest.mark.parametrize("ft,cbound", [(1e-6, 1e-6), (1e-10, 1e-8)])
def test_gpu_pn_wide_feasible(tog, oracle, gpu, ft, cbound):
    """:feasible on the three wide starts: parity, no TRAJ_PN_ERROR and no TRAJ_PN_BLOCK, and c_max below 1e-6
    (ft = 1e-6) / 1e-8 (ft = 1e-10, up to 30 projections and 46 line searches), as on the oracle."""
    gp, st, raised = compare(tog, oracle, WIDE3, pn_opts(tog, ft))
    assert raised is None
    assert not np.any(st["flags"] & (tog.abi.TRAJ_PN_ERROR | tog.abi.TRAJ_PN_BLOCK))
    assert np.all(st["c_max"] < cbound)


@pytest.mark.gpu
def test_gpu_pn_wide_mixed_batch(tog, oracle, gpu):
    """(wide, narrow, wide, narrow): parity for all four, no TRAJ_PN_BLOCK, and the two narrow trajectories come
    out bit-equal to a device solve of those two alone: the second pass does not disturb them."""
    opts = pn_opts(tog, 1e-6)
    parts = [("wide", 0), ("narrow", 0), ("wide", 1), ("narrow", 1)]
    gp, st, raised = compare(tog, oracle, parts, opts)
    assert raised is None
    g2, s2, r2 = device_pn(tog, pick(tog, [("narrow", 0), ("narrow", 1)]), opts)
    assert r2 is None
    for b2, b in enumerate((1, 3)):
        assert np.array_equal(gp._X[b], g2._X[b2]) and np.array_equal(gp._U[b], g2._U[b2]), b
        for key in ("projections", "linesearches", "refinements", "iterations", "c_max", "cost", "viol", "flags"):
            assert st[key][b] == s2[key][b2], (b, key)


@pytest.mark.gpu
def test_gpu_pn_wide_optimal(tog, oracle, gpu):
    """:optimal, one newton step: Y Yᵀ of coincident rows is singular, so both sides end in the reference's
    exception; parity of the iterate and every statistic, equal TRAJ_PN_ERROR flags, no TRAJ_PN_BLOCK."""
    compare(tog, oracle, WIDE3, pn_opts(tog, 1e-8, solve_type="optimal", n_steps=1))


@pytest.mark.gpu
def test_gpu_altro_pn_wide(tog, oracle, gpu):
    """ALTRO end to end on the three wide starts: AL to 1e-3 and the projection on the same device buffers, the
    oracle running the same two phases; no ProjectedNewtonError is raised."""
    prob = wide_problem(tog, wide_starts(), np.zeros((3, NX)))
    opts = tog.ALTROSolverOptions(opts_al=T.car_al_opts(tog, tol=1e-3), projected_newton=True,
                                  projected_newton_tolerance=1e-3)
    opts.opts_pn.active_set_tolerance = 1e-4
    opts.opts_pn.n_steps = 3
    gp = prob.copy()
    solver = tog.solve_b(gp, opts)  # raises ProjectedNewtonError on a flagged trajectory
    flags = solver.stats_pn["flags"]
    assert not np.any(flags & (tog.abi.TRAJ_PN_ERROR | tog.abi.TRAJ_PN_BLOCK))
    for b in range(prob.B):
        o = oracle.OracleSolver(prob, opts.opts_al, b=b)
        o.solve()
        out = o.solve_pn(opts.opts_pn)
        assert T.rel(gp._X[b], o.get("X")) < TOL_STEP and T.rel(gp._U[b], o.get("U")) < TOL_STEP, b
        assert solver.stats_pn["iterations"][b] == out[tog.abi.PN_STEPS]
        assert abs(solver.stats_pn["c_max"][b] - out[tog.abi.PN_C_MAX]) <= 1e-13
