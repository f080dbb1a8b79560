"""Step-level parity of the convergence tail's line-search rollouts (csrc/tog_kernels.hpp; DESIGN.md §5 "tail"):
the three-wave k_ls_spec_tail2, the one-wave k_ls_spec_tail and the bulk k_ls_spec / k_ls_spec_w1 under the tail
flag, each against the CPU oracle on one forward pass. Row counts per knot go up to SPEC_TAIL_PMAX = 16 on both
staged kernels (the quadrotor's 27 staging registers per lane all in use; the Kuka's 64,128-byte image, the largest
that launches) and to 17 on both bulk kernels.

Recipe (test_gpu_parity.py::test_forward_pass_parity with the tail flag of test_qr_column_step.py): solve_step(0)
sets the tail flag and ls_first = nc, so every trial runs in one round; then rollout_open_loop, jacobians,
backward_pass, cost, forward_pass. The device's backward pass is held to the oracle's at TOL_STEP, then both sides
take the oracle's K, d and ΔV, and multipliers that differ per knot and row, so the forward pass runs from
identical inputs. J, X̄, Ū, α, z, the trial count and the cost-increased flag must then equal the oracle's
(oc_forward) bit for bit.

Steering the accepted trial: after the backward pass d is scaled by 2**s per trajectory (exact). Device trial j
then rolls out the unscaled trial j - s; the larger trials overshoot (cost above J_prev) or trip
max_state_value. A trajectory with J_prev = -1 never accepts and runs out of trials (α = 0, X̄ = X). The
conditions the cases cover between them (every one asserted on the oracle, test_cases_cover_the_conditions, on the
CPU):
accepted indices 0, 1 and one in each of 2-7, 8-20, 21-31, 32-40; a trial that diverges before the accepted one;
a divergence at a step that is no multiple of 4 (inside a ring group of k_ls_spec_tail2); a trajectory that runs
out of trials; an AL batch whose trajectories accept different trials in one launch.

Horizons: N - 1 in {1, 3, 5, 15, 16, 17, 33} for the models staged 16 knots at a time (quadrotor, cartpole) and
{7, 8, 9, 17} for the Kuka (8 knots at a time): less than one ring group of 4 steps, non-multiples of 4, exactly
one staging chunk, one more than a chunk, two chunks and one.

The chosen s per case and the trial each trajectory accepts (-2: out of trials), from the oracle:
    quad_rk4_ilqr_1            s = [0, 1, 3]              accepts [0, 1, 2]
    quad_rk4_al_3              s = [0, 2, 9, 5]           accepts [3, 5, 11, -2]
    quad_rk3_al_5              s = [1, 6, 0, 13]          accepts [2, 7, -2, 15]
    quad_rk4_ilqr_15           s = [0, 4, 17]             accepts [2, 5, 19]
    quad_rk4_al_16             s = [3, 0, 11, 19]         accepts [3, 1, 11, 19]
    quad_rk3_sparse_17         s = [0, 7, 2, 15]          accepts [0, 7, 2, 16]
    quad_rk4_al_33             s = [1, 10, 0, 18, 5]      accepts [1, 10, -2, 19, 5]
    quad_rk3_sparse_33         s = [8, 0, 14]             accepts [9, 1, 18]
    quad_rk4_al_17_nc32        s = [22, 27, 30, 0]        accepts [22, 27, 30, 0]
    quad_rk4_rows16_17         s = [0, 6, 13, 3]          accepts [0, 6, 13, 3]
    quad_rk3_rows16_33_nc41    s = [2, 26, 34]            accepts [3, 27, 38]
    quad_rk4_wide_17           s = [0, 6, 12]             accepts [0, 7, 12]
    quad_rk4_al_17_nc41        s = [24, 31, 35, 38, 2]    accepts [25, 31, 35, 39, 3]
    quad_rk3_sparse_33_nc41    s = [33, 29, 39]           accepts [34, 30, -2]
    quad_rk3_inf_17            s = [0, 5, 12]             accepts [0, 5, 11]
    cartpole_mid_uncon_16      s = [0, 3, 10]             accepts [2, 5, 12]
    cartpole_mid_al_5          s = [2, 0, 16]             accepts [7, 5, -2]
    cartpole_mid_al_33         s = [0, 9, 4]              accepts [2, 11, 6]
    kuka_rk3_goal_7            s = [0, 4, 11]             accepts [2, 7, 13]
    kuka_rk3_goal_8            s = [1, 0, 8]              accepts [3, 2, 9]
    kuka_rk3_goal_9            s = [6, 14, 0]             accepts [8, 16, -2]
    kuka_rk3_goal_17           s = [0, 2, 17]             accepts [1, 4, 19]
    kuka_rk3_rows16_17         s = [0, 5, 12]             accepts [4, 8, -2]
    kuka_rk3_wide_9            s = [0, 3, 10]             accepts [2, 5, 12]
"""
import numpy as np
import pytest

TOL_STEP = 1e-13
HOVER = 0.5 * 9.81 / 4


def rel(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    scale = max(1.0, float(np.max(np.abs(b)))) if b.size else 1.0
    return float(np.max(np.abs(a - b))) / scale if b.size else 0.0


# name: model, integrator, mode, steps = N - 1, nc = iterations_linesearch + 1, s per trajectory (B = len(s)),
# jprev = {trajectory: J_prev override}, kernel the launch takes (tog_rollout_plan), win = the oracle's accepted
# trial per trajectory (-2: out of trials).
# modes: "ilqr" constrained problem, iLQR rollouts (no λ, μ image); "uncon" no rows at all; "al" bounds on every
# stage knot + terminal goal; "sparse" a sphere on knots 4-9 and a state row at knots 1 and N - 2 only (kcnt = 0
# elsewhere) + terminal goal; "rows16" control bounds and state rows, 16 per stage knot (SPEC_TAIL_PMAX: the most
# the staged kernels take); "wide" the same with 17 (the bulk kernel); "goal" the terminal goal only; "inf" the
# infeasible-start problem of "goal" (13 slack rows per stage knot, m = 17: the three-wave image is above 64 KB)
# pmax: the most rows on one knot (asserted on the oracle's count, test_cases_cover_the_conditions)
PMAX = {("quad", "ilqr"): 13, ("quad", "al"): 13, ("quad", "sparse"): 13, ("quad", "rows16"): 16, ("quad", "wide"): 17,
        ("quad", "inf"): 13, ("cartpole", "uncon"): 0, ("cartpole", "al"): 4, ("kuka", "goal"): 14,
        ("kuka", "rows16"): 16, ("kuka", "wide"): 17}


def _c(model, integ, mode, steps, nc, s, kernel, win, jprev=None):
    return dict(model=model, integ=integ, mode=mode, steps=steps, nc=nc, s=s, kernel=kernel, win=win,
                jprev=jprev or {}, pmax=PMAX[(model, mode)])


CASES = {
    "quad_rk4_ilqr_1": _c("quad", "rk4", "ilqr", 1, 21, [0, 1, 3], "TAIL3", [0, 1, 2]),
    "quad_rk4_al_3": _c("quad", "rk4", "al", 3, 21, [0, 2, 9, 5], "TAIL3", [3, 5, 11, -2]),
    "quad_rk3_al_5": _c("quad", "rk3", "al", 5, 21, [1, 6, 0, 13], "TAIL3", [2, 7, -2, 15], {2: -1.0}),
    "quad_rk4_ilqr_15": _c("quad", "rk4", "ilqr", 15, 21, [0, 4, 17], "TAIL3", [2, 5, 19]),
    "quad_rk4_al_16": _c("quad", "rk4", "al", 16, 21, [3, 0, 11, 19], "TAIL3", [3, 1, 11, 19]),
    "quad_rk3_sparse_17": _c("quad", "rk3", "sparse", 17, 21, [0, 7, 2, 15], "TAIL3", [0, 7, 2, 16]),
    "quad_rk4_al_33": _c("quad", "rk4", "al", 33, 21, [1, 10, 0, 18, 5], "TAIL3", [1, 10, -2, 19, 5], {2: -1.0}),
    "quad_rk3_sparse_33": _c("quad", "rk3", "sparse", 33, 21, [8, 0, 14], "TAIL3", [9, 1, 18]),
    "quad_rk4_al_17_nc32": _c("quad", "rk4", "al", 17, 32, [22, 27, 30, 0], "TAIL3", [22, 27, 30, 0]),
    "quad_rk4_rows16_17": _c("quad", "rk4", "rows16", 17, 21, [0, 6, 13, 3], "TAIL3", [0, 6, 13, 3]),
    "quad_rk3_rows16_33_nc41": _c("quad", "rk3", "rows16", 33, 41, [2, 26, 34], "TAIL1", [3, 27, 38]),
    "quad_rk4_wide_17": _c("quad", "rk4", "wide", 17, 21, [0, 6, 12], "BULK", [0, 7, 12]),
    "quad_rk4_al_17_nc41": _c("quad", "rk4", "al", 17, 41, [24, 31, 35, 38, 2], "TAIL1", [25, 31, 35, 39, 3]),
    "quad_rk3_sparse_33_nc41": _c("quad", "rk3", "sparse", 33, 41, [33, 29, 39], "TAIL1", [34, 30, -2], {2: -1.0}),
    "quad_rk3_inf_17": _c("quad", "rk3", "inf", 17, 21, [0, 5, 12], "TAIL1", [0, 5, 11]),
    "cartpole_mid_uncon_16": _c("cartpole", "midpoint", "uncon", 16, 21, [0, 3, 10], "TAIL3", [2, 5, 12]),
    "cartpole_mid_al_5": _c("cartpole", "midpoint", "al", 5, 21, [2, 0, 16], "TAIL3", [7, 5, -2]),
    "cartpole_mid_al_33": _c("cartpole", "midpoint", "al", 33, 21, [0, 9, 4], "TAIL3", [2, 11, 6]),
    "kuka_rk3_goal_7": _c("kuka", "rk3", "goal", 7, 21, [0, 4, 11], "TAIL3", [2, 7, 13]),
    "kuka_rk3_goal_8": _c("kuka", "rk3", "goal", 8, 21, [1, 0, 8], "TAIL3", [3, 2, 9]),
    "kuka_rk3_goal_9": _c("kuka", "rk3", "goal", 9, 21, [6, 14, 0], "TAIL3", [8, 16, -2], {2: -1.0}),
    "kuka_rk3_goal_17": _c("kuka", "rk3", "goal", 17, 21, [0, 2, 17], "TAIL3", [1, 4, 19]),
    "kuka_rk3_rows16_17": _c("kuka", "rk3", "rows16", 17, 21, [0, 5, 12], "TAIL3", [4, 8, -2]),
    "kuka_rk3_wide_9": _c("kuka", "rk3", "wide", 9, 21, [0, 3, 10], "BULK_W1", [2, 5, 12]),
}


def _discretize(tog, name, dyn):
    return {"rk3": tog.rk3, "rk4": tog.rk4, "midpoint": tog.midpoint}[name](dyn)


def _options(tog, case, al):
    il = tog.iLQRSolverOptions(square_root=True, iterations_linesearch=case["nc"] - 1)
    return tog.AugmentedLagrangianSolverOptions(opts_uncon=il) if al else il


def build(tog, case):
    """(problem, options, al) of a case; an infeasible-start case's problem carries its slack controls' guess X."""
    N, B, mode = case["steps"] + 1, len(case["s"]), case["mode"]
    rng = np.random.default_rng(100 + case["steps"])
    al = mode not in ("ilqr", "uncon")
    cons = tog.Constraints(N)
    if case["model"] == "quad":
        n, m, dt = 13, 4, 0.05
        x0 = np.zeros((B, n))
        x0[:, 3] = 1.0
        x0[:, :3] += 0.3 * rng.standard_normal((B, 3))
        xf = np.zeros(n)
        xf[3] = 1.0
        xf[:3] = [0.0, 0.04 * case["steps"], 0.0]
        U0 = HOVER + 0.1 * rng.standard_normal((B, N - 1, m))
        model = _discretize(tog, case["integ"], tog.Dynamics.quadrotor)
        obj = tog.LQRObjective(1e-2 * np.eye(n), 1e-2 * np.eye(m), 1000.0 * np.eye(n), xf, N)
        bnd = tog.BoundConstraint(n, m, u_min=0.0, u_max=15.0)
        if mode in ("ilqr", "al"):
            for k in range(N - 1):
                cons[k] += bnd
        elif mode in ("rows16", "wide"):  # 4 + 4 control rows and 8 or 9 state rows: 16 or 17 per stage knot
            x_max = np.full(n, np.inf)
            x_max[[0, 1, 2, 7, 8, 9, 10, 11, 12][: 8 if mode == "rows16" else 9]] = 30.0
            wide = tog.BoundConstraint(n, m, u_min=0.0, u_max=15.0, x_max=x_max)
            for k in range(N - 1):
                cons[k] += wide
        elif mode == "sparse":
            sph = tog.SphereConstraints(n, m, [(0.3, 0.2, 0.1, 0.25)], "obs")
            x_max = np.full(n, np.inf)
            x_max[2] = 0.5
            row = tog.BoundConstraint(n, m, x_max=x_max)
            for k in range(4, min(10, N - 1)):
                cons[k] += sph
            cons[1] += row
            cons[N - 2] += row
        cons[N - 1] += tog.goal_constraint(xf)
        prob = tog.Problem(model, obj, U0, x0=x0, xf=xf, N=N, dt=dt, constraints=cons)
        if mode == "inf":
            t = np.linspace(0.0, 1.0, N)[None, :, None]
            prob.X = x0[:, None, :] + (xf - x0)[:, None, :] * t
            prob = tog.infeasible_problem(prob, 1.0)
    elif case["model"] == "cartpole":
        n, m, dt = 4, 1, 0.05
        xf = np.array([0.0, np.pi, 0.0, 0.0])
        U0 = 0.01 + 0.5 * rng.standard_normal((B, N - 1, m))
        model = _discretize(tog, case["integ"], tog.Dynamics.cartpole)
        obj = tog.LQRObjective(1e-2 * np.eye(n), 1e-1 * np.eye(m), 100.0 * np.eye(n), xf, N)
        if mode == "al":
            bnd = tog.BoundConstraint(n, m, u_min=-3.0, u_max=3.0)
            for k in range(N - 1):
                cons[k] += bnd
            cons[N - 1] += tog.goal_constraint(xf)
        x0 = 0.1 * rng.standard_normal((B, n))
        prob = tog.Problem(model, obj, U0, x0=x0, xf=xf, N=N, dt=dt, constraints=cons)
    else:
        n, m, dt = 14, 7, 0.1
        x0 = np.zeros((B, n))
        x0[:, :7] = rng.uniform(-0.2, 0.2, (B, 7))
        U0 = np.stack([tog.problems.hold_trajectory(n, m, N, tog.Dynamics.kuka, x0[b, :7])[: N - 1] for b in range(B)])
        prob = tog.Problems.kuka(x0=x0, U0=U0, N=N, tf=dt * (N - 1))
        if mode in ("rows16", "wide"):  # 7 + 7 torque rows and 2 or 3 joint-velocity rows: 16 or 17 per stage knot
            x_max = np.full(n, np.inf)
            x_max[7: 9 if mode == "rows16" else 10] = 20.0
            bnd = tog.BoundConstraint(n, m, u_min=-300.0, u_max=300.0, x_max=x_max)
            for k in range(N - 1):
                cons[k] += bnd
            cons[N - 1] += tog.goal_constraint(prob.xf)
            prob = tog.Problem(prob.model, prob.obj, U0, constraints=cons, x0=x0, xf=prob.xf, N=N, dt=prob.dt)
    return prob, _options(tog, case, al), al


def _multipliers(case, shape):
    """λ, μ that differ per knot and row, so a staged multiplier of the wrong knot or row changes the cost:
    λ in [0, 1) with a third of the entries zero (the active-set test reads λ > 0), μ in [0.5, 2)."""
    rng = np.random.default_rng(7 + case["steps"])
    lam = rng.uniform(0.0, 1.0, shape) * (rng.uniform(0.0, 1.0, shape) > 1.0 / 3.0)
    return lam, rng.uniform(0.5, 2.0, shape)


def _divergence_step(o, opts_il):
    """The step (k - 1, producing knot k) at which the oracle's last rollout left max_state_value /
    max_control_value (oc_rollout's own test; the knots after it are stale)."""
    Xb, Ub = o.get("Xbar"), o.get("Ubar")
    for k in range(1, Xb.shape[0]):
        a, u = np.abs(Xb[k]), np.abs(Ub[k - 1])
        if np.isnan(a).any() or np.isnan(u).any() or not (a.max() < opts_il.max_state_value and
                                                        u.max() < opts_il.max_control_value):
            return k - 1
    raise AssertionError("the rollout did not diverge")


_REF = {}


def reference(tog, oracle, name):
    """The oracle's forward pass of every trajectory of a case, computed once: its inputs (K, d scaled, ΔV, λ, μ,
    J_prev), its results, and per trial whether it diverged and at which step (the loop of oc_forward restated
    over oc_rollout and the cost of its X̄, Ū, then checked against oc_forward itself)."""
    if name in _REF:
        return _REF[name]
    case = CASES[name]
    prob, opts, al = build(tog, case)
    il = opts.opts_uncon if al else opts
    out = dict(prob=prob, opts=opts, al=al, traj=[])
    for b, s in enumerate(case["s"]):
        o = oracle.OracleSolver(prob, opts, b=b)
        if case["mode"] == "inf":
            o.slack_controls()
        o.rollout_open_loop()
        if al:
            o.update_constraints()
        o.jacobians()
        assert o.cost_expansion(True, al) == 0
        dV, _ = o.backward(True)
        d = o.get("d") * 2.0 ** s
        o.set("d", d)
        lam = mu = None
        if al:
            lam, mu = _multipliers(case, o.shape("lambda"))
            o.set("lambda", lam)
            o.set("mu", mu)
        J0 = o.cost(al)
        J_prev = case["jprev"].get(b, J0)
        # oc_forward's loop, trial by trial
        diverged, win, J, z = [], -2, np.inf, -1.0
        for j in range(case["nc"]):
            if not ((z <= il.line_search_lower_bound or z > il.line_search_upper_bound) and J >= J_prev):
                break
            alpha = 2.0 ** -j
            if not o.rollout(alpha):
                diverged.append((j, _divergence_step(o, il)))
                continue
            J = o.cost_bar(al)
            expected = -alpha * (dV[0] + alpha * dV[1])
            z = (J_prev - J) / expected if expected > 0.0 else -1.0
            win = j
        if (z <= il.line_search_lower_bound or z > il.line_search_upper_bound) and J >= J_prev:
            win = -2  # out of trials
        Jf = o.forward(J_prev, al)
        st = o.get("stats")
        A = tog.abi
        assert st[A.STAT_ALPHA] == (0.0 if win == -2 else 2.0 ** -win), (name, b)
        if win >= 0:
            assert Jf == J, (name, b)
        out["traj"].append(dict(K=o.get("K"), d=d, dV=np.array(dV), lam=lam, mu=mu, X=o.get("X"), U=o.get("U"),
                                J0=J0, J_prev=J_prev, J=Jf, Xbar=o.get("Xbar"), Ubar=o.get("Ubar"),
                                alpha=st[A.STAT_ALPHA], z=st[A.STAT_Z], trials=st[A.STAT_LS_TRIALS],
                                increased=int(st[A.STAT_FLAGS]) & A.TRAJ_COST_INCREASED, win=win,
                                diverged=diverged))
    out["pmax"] = o.pmax
    _REF[name] = out
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_case_accepts_the_documented_trials(tog, oracle, name):
    """(CPU) the oracle accepts the trials the table above lists, so a case that drifts fails here."""
    ref = reference(tog, oracle, name)
    assert [t["win"] for t in ref["traj"]] == CASES[name]["win"]
    for t in ref["traj"]:
        if t["win"] == -2:  # the fallback: α = 0, X̄ = X
            assert t["alpha"] == 0.0 and np.array_equal(t["Xbar"], t["X"]) and np.array_equal(t["Ubar"], t["U"])


def test_cases_cover_the_conditions(tog, oracle):
    """(CPU) the coverage the module docstring promises, on the oracle's results."""
    refs = {name: reference(tog, oracle, name) for name in CASES}
    wins = {t["win"] for r in refs.values() for t in r["traj"]}
    assert 0 in wins and 1 in wins
    for lo, hi in ((2, 7), (8, 20), (21, 31), (32, 40)):
        assert any(lo <= w <= hi for w in wins), (lo, hi)
    # the three-wave kernel's upper lanes, and the one-wave kernel's past the 32nd
    assert any(21 <= t["win"] <= 31 for n, r in refs.items() if CASES[n]["kernel"] == "TAIL3" for t in r["traj"])
    assert any(t["win"] >= 32 for n, r in refs.items() if CASES[n]["kernel"] == "TAIL1" for t in r["traj"])
    div = [(j, step, t["win"]) for r in refs.values() for t in r["traj"] for j, step in t["diverged"]]
    assert any(w >= 0 and j < w for j, _, w in div)  # a diverged trial before the accepted one
    assert any(step % 4 != 0 for _, step, _ in div)  # a divergence inside a ring group
    assert -2 in wins  # out of trials
    assert any(r["al"] and len({t["win"] for t in r["traj"]}) > 1 for r in refs.values())  # mixed outcomes, AL
    # every kernel, every horizon of the docstring
    assert {c["kernel"] for c in CASES.values()} == {"TAIL3", "TAIL1", "BULK", "BULK_W1"}
    # the most rows per knot the staged kernels take, on both of them under AL, and one more on both bulk kernels
    assert all(r["pmax"] == CASES[n]["pmax"] for n, r in refs.items())
    for kernel, pmax, models in (("TAIL3", 16, {"quad", "kuka"}), ("TAIL1", 16, {"quad"}), ("BULK", 17, {"quad"}),
                                 ("BULK_W1", 17, {"kuka"})):
        assert {c["model"] for n, c in CASES.items()
                if c["kernel"] == kernel and c["pmax"] == pmax and refs[n]["al"]} == models, (kernel, pmax)
    assert {c["steps"] for c in CASES.values() if c["model"] != "kuka"} >= {1, 3, 5, 15, 16, 17, 33}
    assert {c["steps"] for c in CASES.values() if c["model"] == "kuka"} >= {7, 8, 9, 17}
    # rows on some stage knots only: kcnt = 0 elsewhere
    nc = refs["quad_rk3_sparse_17"]["prob"].constraints.num_constraints()
    assert nc[0] == 0 and nc[1] == 1 and nc[2] == 0 and nc[4] == 1 and nc[16] == 1 and nc[17] == 13
    nc = refs["quad_rk4_rows16_17"]["prob"].constraints.num_constraints()
    assert all(c == 16 for c in nc[:-1]) and nc[-1] == 13
    nc = refs["kuka_rk3_rows16_17"]["prob"].constraints.num_constraints()
    assert all(c == 16 for c in nc[:-1]) and nc[-1] == 14


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_tail_forward_pass_equals_oracle(tog, oracle, gpu, name):
    A = tog.abi
    case = CASES[name]
    ref = reference(tog, oracle, name)
    prob, opts, al, trajs = ref["prob"], ref["opts"], ref["al"], ref["traj"]
    B = len(trajs)
    h = tog.AbstractSolverFor(prob, opts).handle
    h.solve_step(0)  # no step: the handle takes the tail flag and one-round line searches of a small batch
    assert h.rollout_plan() == getattr(A, "ROLLOUT_" + case["kernel"]), "the case runs another kernel than it means to"
    if case["mode"] == "inf":
        h.slack_controls()
    h.rollout_open_loop()
    h.jacobians()
    dV = h.backward_pass(sqrt=True, al=al)
    K, d = h.get(A.FIELD_K), h.get(A.FIELD_D)
    for b, t in enumerate(trajs):
        assert np.array_equal(h.get(A.FIELD_X)[b], t["X"]) and np.array_equal(h.get(A.FIELD_U)[b], t["U"]), b
        errs = (rel(dV[b], t["dV"]), rel(K[b], t["K"]), rel(d[b] * 2.0 ** case["s"][b], t["d"]))
        assert max(errs) < TOL_STEP, (b, errs)
    # identical gains on both sides: the oracle's K and ΔV, its d scaled by 2**s
    h.set(A.FIELD_K, np.stack([t["K"] for t in trajs]))
    h.set(A.FIELD_D, np.stack([t["d"] for t in trajs]))
    h.set(A.FIELD_DV, np.stack([t["dV"] for t in trajs]))
    if al:
        h.set(A.FIELD_LAMBDA, np.stack([t["lam"] for t in trajs]))
        h.set(A.FIELD_MU, np.stack([t["mu"] for t in trajs]))
    J0 = h.cost(al=al)
    assert np.array_equal(J0, [t["J0"] for t in trajs])
    J = h.forward_pass(np.array([t["J_prev"] for t in trajs]), al=al)
    Xb, Ub, st = h.get(A.FIELD_XBAR), h.get(A.FIELD_UBAR), h.get(A.FIELD_STATS)
    for b, t in enumerate(trajs):
        got = (J[b], st[b, A.STAT_ALPHA], st[b, A.STAT_Z], st[b, A.STAT_LS_TRIALS],
               int(st[b, A.STAT_FLAGS]) & A.TRAJ_COST_INCREASED)
        want = (t["J"], t["alpha"], t["z"], t["trials"], t["increased"])
        print(f"{name} b={b} win={t['win']}: J {got[0]!r} / {want[0]!r}, alpha {got[1]} / {want[1]}, "
              f"X̄ {rel(Xb[b], t['Xbar']):.3e}, Ū {rel(Ub[b], t['Ubar']):.3e}")
        assert got == want, (b, got, want)
        assert np.array_equal(Ub[b], t["Ubar"]), (b, rel(Ub[b], t["Ubar"]))
        assert np.array_equal(Xb[b], t["Xbar"]), (b, rel(Xb[b], t["Xbar"]))
