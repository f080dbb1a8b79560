"""The Householder column step of team_qr (csrc/tog_bwd_team.hpp) in its second form (wave A's QRs in k_bwd_quad):
the pivot's reciprocal is computed on every lane and selected, without the exec branch around the division
(DESIGN.md §5). Every live lane performs the same operations on the same values in the same order as in the first
form, so every backward kernel still equals the CPU oracle bit for bit, whichever form its QRs take.

Step level: one Jacobian, expansion and square-root backward pass against the oracle (K, d, ΔV to TOL_STEP, as
tests/test_gpu_parity.py), on the kernel a step-level call takes (k_bwd_team) and, once the handle carries the tail
flag, on the four-wave k_bwd_quad. Solve level: a config-3 batch on the default plan equals the same batch on the
one-wave team kernel and the oracle's solves. Restarts: a control cost whose Q.uu factor has a condition number
above 1e8 makes every backward pass increase the regularisation and start again, so the released rows of a
discarded attempt and the faithful replay run.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_STEP = 1e-13


def rel(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    scale = max(1.0, float(np.max(np.abs(b)))) if b.size else 1.0
    return float(np.max(np.abs(a - b))) / scale if b.size else 0.0


def _env(env):
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    return old


def _config3(tog, B):
    return tog.Problems.config_quadrotor(B=B)


def _config3_varying(tog, B):
    """config 3 under a time-varying Objective: LQRCost(Q w_k, R v_k, xf) per knot, weights ramping along the
    horizon (the TV kernel variants)."""
    prob, opts = tog.Problems.config_quadrotor(B=B)
    st, term = prob.obj.stage, prob.obj.terminal
    N = prob.N
    costs = [tog.LQRCost((0.5 + 1.5 * k / (N - 2)) * st.Q, (2.0 - 1.0 * k / (N - 2)) * st.R, prob.xf)
             for k in range(N - 1)]
    obj = tog.Objective(costs + [tog.LQRCostTerminal(term.Q, prob.xf)])
    p = tog.Problem(prob.model, obj, prob._U.copy(), constraints=prob.constraints, x0=prob.x0.copy(), xf=prob.xf,
                    N=prob.N, dt=prob.dt)
    p._X[...] = prob._X
    return p, opts


def _cartpole(tog, B):
    prob, opts = tog.Problems.config_cartpole(B=B)
    opts.square_root = True
    return prob, opts


# (problem, B, AL expansion, 16-lane teams: the tail flag then selects k_bwd_quad)
STEP_CASES = {"config3": (_config3, 5, True, True), "config3_varying": (_config3_varying, 4, True, True),
              "cartpole": (_cartpole, 3, False, False)}
_REF = {}


def _step_reference(tog, oracle, case):
    """The oracle's backward pass of every trajectory of a case, computed once."""
    if case not in _REF:
        make, B, al, _ = STEP_CASES[case]
        prob, opts = make(tog, B)
        out = []
        for b in range(B):
            o = oracle.OracleSolver(prob, opts, b=b)
            o.rollout_open_loop()
            if al:
                o.update_constraints()
            o.jacobians()
            assert o.cost_expansion(True, al) == 0
            dV, _ = o.backward(True)
            out.append((np.array(dV), o.get("K").copy(), o.get("d").copy()))
        _REF[case] = (prob, opts, out)
    return _REF[case]


@pytest.mark.parametrize("tail", [False, True])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_backward_step_equals_oracle(tog, oracle, gpu, case, tail):
    _, B, al, wide = STEP_CASES[case]
    prob, opts, ref = _step_reference(tog, oracle, case)
    h = tog.AbstractSolverFor(prob, opts).handle
    if tail:
        h.solve_step(0)  # no step: the handle takes the tail flag of a small batch (k_bwd_quad on 16-lane teams)
    h.rollout_open_loop()
    h.jacobians()
    dV = h.backward_pass(sqrt=True, al=al)
    K, d = h.get(tog.abi.FIELD_K), h.get(tog.abi.FIELD_D)
    for b in range(B):
        dV_ref, K_ref, d_ref = ref[b]
        errs = (rel(dV[b], dV_ref), rel(K[b], K_ref), rel(d[b], d_ref))
        print(f"{case} tail={tail} wide={wide} b={b}: dV {errs[0]:.3e} K {errs[1]:.3e} d {errs[2]:.3e}")
        assert max(errs) < TOL_STEP, (b, errs)


def _solve(tog, make, env):
    old = _env(env)
    try:
        prob, opts = make()
        gpu = prob.copy()
        solver = tog.solve_b(gpu, opts)
        return prob, opts, gpu._X.copy(), gpu._U.copy(), solver.handle.get(tog.abi.FIELD_STATS)
    finally:
        _env(old)


def test_config3_solve_default_team_oracle(tog, oracle, gpu):
    """Config 3 at B = 8 to convergence: the default plan (k_bwd_quad), the one-wave k_bwd_team and the oracle
    agree in X, U, iterations and flags."""
    A = tog.abi
    B = 8
    prob, opts, Xa, Ua, Sa = _solve(tog, lambda: tog.Problems.config_quadrotor(B=B), {"TOG_BWD_TAIL": None})
    _, _, Xb, Ub, Sb = _solve(tog, lambda: tog.Problems.config_quadrotor(B=B), {"TOG_BWD_TAIL": "team"})
    assert np.array_equal(Xa, Xb) and np.array_equal(Ua, Ub) and np.array_equal(Sa, Sb)
    assert not (Sa[:, A.STAT_FLAGS].astype(np.int64) & A.TRAJ_ACTIVE).any()  # solved to the end

    def run(b):
        o = oracle.OracleSolver(prob, opts, b=b)
        steps = o.solve()
        return steps, o.get("X"), o.get("U"), o.get("stats")

    with ThreadPoolExecutor(max_workers=B) as ex:  # (ctypes releases the GIL)
        results = list(ex.map(run, range(B)))
    for b, (steps, X, U, st) in enumerate(results):
        assert steps == int(Sa[b, A.STAT_TOTAL_STEPS]), b
        assert int(st[A.STAT_FLAGS]) == int(Sa[b, A.STAT_FLAGS]), b
        assert np.array_equal(Xa[b], X) and np.array_equal(Ua[b], U), b


def _restart_problem(tog, varying, N=31):
    """The quadrotor of tests/test_pd_exception.py (one trajectory, N = 31, rk3, dt = 0.05) with a control cost
    R = diag(1, 1, 1, 1e-17) and state costs of 1e-20: Q.uu ≈ R dt, whose factor's condition number 3.2e8 is above
    the 1e8 bound of backward_pass.jl:129, so the pass increases ρ and starts again. `varying`: only the knots
    before k = 12 carry that R (a time-varying Objective), so the attempt is discarded in the middle of the horizon
    after 18 accepted knots."""
    n, m = 13, 4
    x0 = np.zeros(n)
    x0[3] = 1.0
    xf = x0.copy()
    xf[0] = 1.0
    bad = np.diag([1.0, 1.0, 1.0, 1e-17])
    Q, H = 1e-20 * np.eye(n), np.zeros((m, n))
    term = tog.LQRCostTerminal(1e-20 * np.eye(n), xf)
    if varying:
        obj = tog.Objective([tog.QuadraticCost(Q, bad if k < 12 else np.eye(m), H=H) for k in range(N - 1)] + [term])
    else:
        obj = tog.Objective(tog.QuadraticCost(Q, bad, H=H), term, N=N)
    U0 = np.full((N - 1, m), 0.5 * 9.81 / 4 * 0.5)
    return tog.Problem(tog.rk3(tog.Dynamics.quadrotor), obj, U0, x0=x0, N=N, dt=0.05)


@pytest.mark.parametrize("kind", [None, "team"])
@pytest.mark.parametrize("varying", [False, True])
def test_backward_restart_equals_oracle(tog, oracle, gpu, varying, kind):
    A = tog.abi
    opts = tog.iLQRSolverOptions(square_root=True, iterations=50)
    prob = _restart_problem(tog, varying)
    ref = oracle.OracleSolver(prob, opts)
    steps = ref.solve()
    st = ref.get("stats")
    assert steps >= 2 and int(st[A.STAT_BP_RESTARTS]) >= 1  # the case really restarts
    _, _, X, U, S = _solve(tog, lambda: (prob, opts), {"TOG_BWD_TAIL": kind})
    assert int(S[0, A.STAT_TOTAL_STEPS]) == steps
    # (the device's count includes its faithful replay of the attempt that failed first, the oracle's does not)
    assert int(S[0, A.STAT_BP_RESTARTS]) >= int(st[A.STAT_BP_RESTARTS])
    assert int(S[0, A.STAT_FLAGS]) == int(st[A.STAT_FLAGS])
    assert np.array_equal(X[0], ref.get("X")) and np.array_equal(U[0], ref.get("U"))
