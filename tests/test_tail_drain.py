"""The drain between the two QRs of a k_bwd_quad knot (csrc/tog_bwd_quad.hpp, TOG_QUAD_DRAIN): wave D's
branch-free epilogue, its specialised drain steps and tog_rsqrt_select. None of them changes a value a lane computes or
the order of its operations, so the four-wave kernel still equals the one-wave k_bwd_team and the CPU oracle bit for bit.

Solve level: the quadrotor (m = 4, three drain steps) and the Kuka arm (n = 14, m = 7, six drain steps, the widest
epilogue) at 1, 2, 5 and 17 stage knots, one and three trajectories, AL and plain iLQR, square-root passes, solved with
TOG_BWD_TAIL=quad and =team: X, U and every statistic equal bit for bit. Step level: one backward pass under the tail
flag against the oracle's K, d and ΔV. And the two ways out of a knot that a healthy solve never takes, both decided
right behind the B2b barrier from what wave D's epilogue left there: the regularisation restart (tmp2 and the flags of
the dropped knot are on the bus, the lower triangle written once per launch must survive it) and the downdate's
PosDefException (flg[2] set, now by every lane of wave D).
"""
import os

import numpy as np
import pytest

from test_pd_exception import _quad_problem
from test_qr_column_step import TOL_STEP, _restart_problem, rel

pytestmark = pytest.mark.gpu


def _env(env):
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return old


def _quadrotor(tog, N, B, al):
    """tests/test_edge_cases.py's short-horizon quadrotor: rk4, dt = 0.05, the goal 2 m away, jittered starts."""
    rng = np.random.default_rng(100 + N)
    p0 = tog.Problems.quadrotor_test("goal+bounds")
    n, m = 13, 4
    x0 = np.tile(p0.x0[0], (B, 1))
    x0[:, :3] += 0.3 * rng.standard_normal((B, 3))
    xf = p0.xf.copy()
    xf[:3] = [0.0, 2.0, 0.0]
    cons = tog.Constraints(N)
    if al:
        bnd = tog.BoundConstraint(n, m, u_min=0.0, u_max=15.0)
        for k in range(N - 1):
            cons[k] += bnd
        cons[N - 1] += tog.goal_constraint(xf)
    obj = tog.LQRObjective(p0.obj.stage.Q, p0.obj.stage.R, p0.obj.terminal.Q, xf, N)
    U0 = 0.5 * 9.81 / 4 + 0.1 * rng.standard_normal((B, N - 1, m))
    return tog.Problem(p0.model, obj, U0, x0=x0, xf=xf, N=N, dt=0.05, constraints=cons)


def _kuka(tog, N, B, al):
    """The Kuka arm of Problems.kuka (rk3, dt = 0.1, hold-trajectory controls) from jittered joint angles; the
    terminal goal constraint only with AL."""
    n, m = 14, 7
    x0 = np.zeros((B, n))
    for b in range(B):
        x0[b, :7] = np.random.default_rng(200 + N + b).uniform(-0.2, 0.2, 7)
    U0 = np.stack([tog.Problems.hold_trajectory(n, m, N, tog.Dynamics.kuka, x0[b, :7])[: N - 1] for b in range(B)])
    p = tog.Problems.kuka(x0=x0, U0=U0, N=N, tf=0.1 * (N - 1))
    if al:
        return p
    return tog.Problem(p.model, p.obj, U0, x0=x0, xf=p.xf, N=N, dt=p.dt)


MODELS = {"quadrotor": _quadrotor, "kuka": _kuka}


def _opts(tog, al):
    il = tog.iLQRSolverOptions(square_root=True, iterations=40)
    return tog.AugmentedLagrangianSolverOptions(opts_uncon=il, iterations=4) if al else il


def _solve(tog, prob, opts, kind):
    old = _env({"TOG_BWD_TAIL": kind})
    try:
        s = tog.AbstractSolverFor(prob.copy(), opts)
        h = s.handle
        h.solve(s.mode)
        A = tog.abi
        return h.get(A.FIELD_X, raw=True), h.get(A.FIELD_U, raw=True), h.get(A.FIELD_STATS, raw=True)
    finally:
        _env(old)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("al", [True, False], ids=["al", "ilqr"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("knots", [1, 2, 5, 17])
@pytest.mark.parametrize("model", list(MODELS))
def test_quad_and_team_solves_agree(tog, gpu, model, knots, B, al):
    prob, opts = MODELS[model](tog, knots + 1, B, al), _opts(tog, al)
    Xq, Uq, Sq = _solve(tog, prob, opts, "quad")
    Xt, Ut, St = _solve(tog, prob, opts, "team")
    assert Sq[:, tog.abi.STAT_TOTAL_STEPS].min() >= 1  # the solves really iterated
    assert _same_bits(Xq, Xt) and _same_bits(Uq, Ut) and _same_bits(Sq, St)


@pytest.mark.parametrize("model", list(MODELS))
def test_tail_backward_step_equals_oracle(tog, oracle, gpu, model):
    B, al = 3, True
    prob, opts = MODELS[model](tog, 6, B, al), _opts(tog, al)
    old = _env({"TOG_BWD_TAIL": "quad"})
    try:
        h = tog.AbstractSolverFor(prob, opts).handle
        h.solve_step(0)  # no step: the handle takes the tail flag of a small batch, and the pass k_bwd_quad
        h.rollout_open_loop()
        h.jacobians()
        dV = h.backward_pass(sqrt=True, al=al)
        K, d = h.get(tog.abi.FIELD_K), h.get(tog.abi.FIELD_D)
    finally:
        _env(old)
    for b in range(B):
        o = oracle.OracleSolver(prob, opts, b=b)
        o.rollout_open_loop()
        o.update_constraints()
        o.jacobians()
        assert o.cost_expansion(True, al) == 0
        dV_ref, _ = o.backward(True)
        errs = (rel(dV[b], dV_ref), rel(K[b], o.get("K")), rel(d[b], o.get("d")))
        print(f"{model} b={b}: dV {errs[0]:.3e} K {errs[1]:.3e} d {errs[2]:.3e}")
        assert max(errs) < TOL_STEP, (b, errs)


@pytest.mark.parametrize("varying", [False, True])
def test_restart_equals_team_and_oracle(tog, oracle, gpu, varying):
    """cond(Q.uu) > 1e8 (tests/test_qr_column_step.py's control cost): every pass restarts, with `varying` in the
    middle of the horizon; the attempts after it reuse tmp2's lower triangle, which is written once per launch."""
    A = tog.abi
    opts = tog.iLQRSolverOptions(square_root=True, iterations=50)
    prob = _restart_problem(tog, varying)
    ref = oracle.OracleSolver(prob, opts)
    steps = ref.solve()
    st = ref.get("stats")
    assert steps >= 2 and int(st[A.STAT_BP_RESTARTS]) >= 1  # the case really restarts
    Xq, Uq, Sq = _solve(tog, prob, opts, "quad")
    Xt, Ut, St = _solve(tog, prob, opts, "team")
    assert _same_bits(Xq, Xt) and _same_bits(Uq, Ut) and _same_bits(Sq, St)
    assert int(Sq[0, A.STAT_TOTAL_STEPS]) == steps
    assert int(Sq[0, A.STAT_BP_RESTARTS]) >= int(st[A.STAT_BP_RESTARTS])  # (the device counts its faithful replay too)
    assert int(Sq[0, A.STAT_FLAGS]) == int(st[A.STAT_FLAGS])
    assert np.array_equal(Xq[0], ref.get("X")) and np.array_equal(Uq[0], ref.get("U"))


@pytest.mark.parametrize("hval", [1.1, 2.0])
def test_downdate_failure_flag_reaches_every_wave(tog, oracle, gpu, hval):
    """tests/test_pd_exception.py's quadrotor: the downdate fails at the first pass (h = 2) or after one accepted
    step (h = 1.1); wave D's flg[2], now stored by all of its lanes, stops the trajectory where the oracle stops."""
    A = tog.abi
    opts = tog.iLQRSolverOptions(square_root=True, iterations=50)
    prob = _quad_problem(tog, hval)
    ref = oracle.OracleSolver(prob, opts)
    steps = ref.solve()
    st = ref.get("stats")
    want = A.TRAJ_SQRT_PD_FAIL | A.TRAJ_BP_ABORTED
    assert int(st[A.STAT_FLAGS]) & want == want and steps == (1 if hval == 1.1 else 0)
    Xq, Uq, Sq = _solve(tog, prob, opts, "quad")
    Xt, Ut, St = _solve(tog, prob, opts, "team")
    assert _same_bits(Xq, Xt) and _same_bits(Uq, Ut) and _same_bits(Sq, St)
    assert int(Sq[0, A.STAT_FLAGS]) & want == want  # the oracle's two flags
    assert int(Sq[0, A.STAT_TOTAL_STEPS]) == steps
    assert np.array_equal(Xq[0], ref.get("X")) and np.array_equal(Uq[0], ref.get("U"))
