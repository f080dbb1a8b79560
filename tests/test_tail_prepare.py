"""A tail step's Jacobians and cost expansion as one launch (k_tail_prepare, csrc/tog_bwd_team.hpp; the grid in
tog_plan::tail_prepare; DESIGN.md §5 "One preparation launch"). The fused kernel's blocks run the bodies of k_jacobian,
k_expand_u and k_expand_team on the work items the separate kernels give them, so a solve on either path
(TOG_TAIL_PREPARE=split keeps the three launches) gives the same bits: X, U and every per-trajectory statistic.

Shapes: B in {1, 3, 5} and N - 1 in {1, 5, 17}, the smallest where a block-range boundary or a role's indexing can go
wrong: with the quadrotor's 5 Jacobian chunks per knot and 16 wide teams per block none of B (N-1) 5 is a multiple
of 256, none of B (N-1) a multiple of 64, and neither B nor B N a multiple of 16 (the cartpole's 32 teams per block:
B N is no multiple of 32 either); the ranges are 1 or 2 Jacobian blocks, 1 or 2 blocks of 4-lane teams and 1 to 6
blocks of wide teams (tests/test_prepare_plan.py pins the arithmetic). Problems are the step-level cases of
tests/test_tail_line_search.py (its build()), so every batch is of the tail's size.

Which path ran is read from the profile: a fused step is timed as the Jacobian and records no expansion launch.

One step from identical state against the CPU oracle (Jacobians, gains K, d at the step tolerance of
tests/test_gpu_parity.py, 1e-13) holds the fused kernel to the reference and not only to the split path.
"""
import os

import numpy as np
import pytest

import test_tail_line_search as tls  # (build(): the small quadrotor / cartpole / Kuka problems and their options)

TOL_STEP = 1e-13
JAC, EXPANSION = 0, 3  # tog_kernel_id
SHAPES = [(B, steps) for B in (1, 3, 5) for steps in (1, 5, 17)]


def _case(model, integ, mode, steps, B):
    return dict(model=model, integ=integ, mode=mode, steps=steps, nc=21, s=[0] * B)


def _make(tog, model, integ, mode, steps, B, sqrt=True, variant=None):
    prob, opts, al = tls.build(tog, _case(model, integ, mode, steps, B))
    il = opts.opts_uncon if al else opts
    il.square_root = sqrt
    il.iterations = 25
    if al:
        opts.iterations = 3
    if variant == "goals":  # a goal per trajectory, in the cost and in the goal rows (Problems.config_quadrotor_goals)
        N = prob.N
        XF = np.tile(prob.xf, (B, 1))
        XF[:, 0:3] += np.random.default_rng(31 + steps).uniform(-0.5, 0.5, (B, 3))
        obj = tog.LQRObjectiveBatch(prob.obj.stage.Q, prob.obj.stage.R, prob.obj.terminal.Q, XF, N)
        goal = tog.goal_constraint(XF)
        cons = tog.Constraints(N)
        for k in range(N):
            cons[k] = tog.ConstraintSet(goal if isinstance(c, tog.GoalConstraint) else c for c in prob.constraints[k])
        out = tog.Problem(prob.model, obj, constraints=cons, x0=prob.x0, xf=XF, N=N, dt=prob.dt)
        out._U[...] = prob._U
        prob = out
    elif variant == "tv":  # a stage cost per knot (Problems.config_quadrotor_tv)
        N = prob.N
        st, term = prob.obj.stage, prob.obj.terminal
        costs = [tog.LQRCost((0.5 + 1.5 * k / max(1, N - 2)) * st.Q, (2.0 - k / max(1, N - 2)) * st.R, prob.xf)
                 for k in range(N - 1)]
        obj = tog.Objective(costs + [tog.LQRCostTerminal(term.Q, prob.xf)])
        prob = tog.Problem(prob.model, obj, prob._U.copy(), constraints=prob.constraints, x0=prob.x0.copy(),
                           xf=prob.xf, N=N, dt=prob.dt)
    return prob, opts, al


def _env(env):
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return old


def _solve(tog, prob, opts, al, env, checks=None):
    """tog_solve's loop (chunks of 4 steps and a stopping check) with the profile on: X, U, statistics rows, the
    launch counts per kernel id and the active counts the checks returned."""
    A = tog.abi
    old = _env(env)
    try:
        h = tog.AbstractSolverFor(prob.copy(), opts).handle
        h.solve_init(A.MODE_AL if al else A.MODE_ILQR)
        h.profile(True)
        seen = []
        for _ in range(40):
            h.solve_step(4)
            seen.append(h.batch_stats()[0])
            if seen[-1] == 0.0:
                break
        _, launches = h.profile_read()
        h.profile(False)
        return (h.get(A.FIELD_X), h.get(A.FIELD_U), h.get(A.FIELD_STATS)), launches, seen
    finally:
        _env(old)


def _fused_equals_split(tog, prob, opts, al, fused=True):
    a, la, seen = _solve(tog, prob, opts, al, {"TOG_TAIL_PREPARE": None})
    b, lb, _ = _solve(tog, prob, opts, al, {"TOG_TAIL_PREPARE": "split"})
    assert la[JAC] > 0 and la[JAC] == lb[JAC]
    assert lb[EXPANSION] == lb[JAC]  # the split path: an expansion launch per step
    assert la[EXPANSION] == (0 if fused else la[JAC])  # the default plan: fused, or split where the plan says so
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[2][:, tog.abi.STAT_TOTAL_STEPS].min() >= 1
    return a, seen


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [True, False], ids=["sqrt", "std"])
def test_quadrotor_al(tog, gpu, sqrt):
    """Config 3's problem class (control bounds on every stage knot, terminal goal). sqrt: 4-lane teams for the stage
    knots and the terminal knot on the wide teams; std: every knot on the wide teams."""
    for B, steps in SHAPES:
        _fused_equals_split(tog, *_make(tog, "quad", "rk4", "al", steps, B, sqrt=sqrt))


@pytest.mark.gpu
def test_cartpole_ilqr(tog, gpu):
    """No AL bit, 8-lane teams, one Jacobian chunk per knot."""
    for B, steps in SHAPES:
        _fused_equals_split(tog, *_make(tog, "cartpole", "midpoint", "uncon", steps, B))


@pytest.mark.gpu
def test_quadrotor_state_rows_on_stage_knots(tog, gpu):
    """A state row on stage knots 1 and N - 2 and a sphere on knots 4-9: dense stage knots, which the 4-lane teams skip
    and the wide teams take (mode 1), each skipping the other's knots."""
    for B in (1, 3, 5):
        for steps in (5, 17):
            prob, opts, al = _make(tog, "quad", "rk3", "sparse", steps, B)
            assert prob.constraints.num_constraints()[1] >= 1
            _fused_equals_split(tog, prob, opts, al)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["goals", "tv"])
def test_quadrotor_cost_tables(tog, gpu, variant):
    """goals: per-trajectory goals (the PT bit of the expansion roles); tv: a time-varying objective."""
    for B, steps in ((3, 5), (5, 17), (1, 1)):
        _fused_equals_split(tog, *_make(tog, "quad", "rk4", "al", steps, B, variant=variant))


@pytest.mark.gpu
def test_kuka_stays_split(tog, gpu):
    """The Kuka's Jacobians are a stage chain of four kernels: the plan answers split, and the solve is the same."""
    prob, opts, al = _make(tog, "kuka", "rk3", "goal", 7, 3)
    opts.opts_uncon.iterations = 6
    opts.iterations = 2
    _fused_equals_split(tog, prob, opts, al, fused=False)


@pytest.mark.gpu
def test_inactive_trajectory_and_compacted_launches(tog, gpu):
    """B = 5 with trajectory 2 started at the goal with hover controls, so it finishes first: from then on every
    launch has an inactive trajectory in it, and after the next stopping check the launches go over the list of
    the active ones (last_active < B). Fused equals split, and both equal TOG_NO_COMPACT=1 (no list)."""
    prob, opts, al = _make(tog, "quad", "rk4", "al", 17, 5)
    prob.x0[2] = prob.xf
    prob._U[2] = tls.HOVER
    a, seen = _fused_equals_split(tog, prob, opts, al)
    assert any(0.0 < s < 5.0 for s in seen[:-1]), "no step ran over a list of fewer than B trajectories"
    c, lc, _ = _solve(tog, prob, opts, al, {"TOG_TAIL_PREPARE": None, "TOG_NO_COMPACT": "1"})
    assert lc[EXPANSION] == 0
    for x, y in zip(a, c):
        assert np.array_equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quad_al_sqrt", "quad_al_std", "quad_sparse", "cartpole_ilqr"])
def test_one_fused_step_equals_oracle(tog, oracle, gpu, name):
    model, integ, mode, steps, B, sqrt = {"quad_al_sqrt": ("quad", "rk4", "al", 17, 5, True),
                                          "quad_al_std": ("quad", "rk4", "al", 5, 3, False),
                                          "quad_sparse": ("quad", "rk3", "sparse", 17, 3, True),
                                          "cartpole_ilqr": ("cartpole", "midpoint", "uncon", 17, 5, True)}[name]
    A = tog.abi
    prob, opts, al = _make(tog, model, integ, mode, steps, B, sqrt=sqrt)
    h = tog.AbstractSolverFor(prob.copy(), opts).handle
    h.solve_init(A.MODE_AL if al else A.MODE_ILQR)
    h.profile(True)
    h.solve_step(1)
    _, launches = h.profile_read()
    h.profile(False)
    assert launches[JAC] == 1 and launches[EXPANSION] == 0  # the fused launch
    Ad, Bd, K, d = h.get(A.FIELD_A), h.get(A.FIELD_B), h.get(A.FIELD_K), h.get(A.FIELD_D)
    dyn = {"quad": tog.Dynamics.quadrotor, "cartpole": tog.Dynamics.cartpole}[model]
    n, m, ig = dyn.n, dyn.m, {"rk3": A.RK3, "rk4": A.RK4, "midpoint": A.MIDPOINT}[integ]
    for b in range(B):
        o = oracle.OracleSolver(prob, opts, b=b)
        o.rollout_open_loop()
        if al:
            o.update_constraints()
        o.jacobians()
        assert o.cost_expansion(sqrt, al) == 0
        o.backward(sqrt)
        X, U = o.get("X"), o.get("U")
        for k in range(steps):
            S = oracle.discrete_jacobian(dyn.model_id, ig, X[k], U[k], prob.dt)
            assert tls.rel(Ad[b, k], S[:, :n]) < TOL_STEP and tls.rel(Bd[b, k], S[:, n:n + m]) < TOL_STEP, (b, k)
        errs = (tls.rel(K[b], o.get("K")), tls.rel(d[b], o.get("d")))
        print(f"{name} b={b}: K {errs[0]:.3e}, d {errs[1]:.3e}")
        assert max(errs) < TOL_STEP, (b, errs)
