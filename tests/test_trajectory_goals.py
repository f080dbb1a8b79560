"""Per-trajectory goals and linear cost terms within one batch (tog_set_trajectory_costs, tog_set_trajectory_goals).

The batch shares every cost Hessian; trajectory b has its own [q; r; c] (one row, or one per stage knot), its own
[qf; cf] and its own goal-row targets (DevProblem::lin / term / goal, read by cost_at / term_at / traj_row in
csrc/tog_device.hpp). The oracle solves one trajectory per descriptor, so trajectory b of such a batch is held to
the oracle run on ``prob.trajectory(b)``, the plain single-goal problem of b: X, U within 1e-6 (relative, as
tests/test_time_varying.py), equal iteration counts, and STAT_J within 1e-6 relative. The cost is what catches a
wrong constant term c, which leaves X and U unchanged: for the cartpole goals below it is 1/2 xf'Q xf tf, about
0.25 against costs of order 10, four orders of magnitude above the bound.

Goal sets (seeds frozen): cartpole cart position in +-0.5 m around the swing-up goal, quadrotor goal position
within +-1 m of config 3's. The CPU test ``test_inputs_converge_in_the_oracle`` holds the inputs themselves to the
condition that every trajectory's oracle solve converges within the options' limits with no exception flag.
"""
import ctypes as C
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from test_time_varying import ramp_objective

ROOT = pathlib.Path(__file__).resolve().parent.parent
TOL_SOLVE = 1e-6
TOL_J = 1e-6


def rel(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    scale = max(1.0, float(np.max(np.abs(b)))) if b.size else 1.0
    return float(np.max(np.abs(a - b))) / scale if b.size else 0.0


# ----------------------------------------------------------------------------- problems


def cartpole_goal_set(tog, B, offset=0):
    """XF (B, 4): the swing-up goal with the cart position moved by U(-0.5, 0.5) (seed 4000 + offset + b)."""
    prob, _ = tog.Problems.config_cartpole(B=1)
    d = np.stack([np.random.default_rng(4000 + offset + b).uniform(-0.5, 0.5) for b in range(B)])
    XF = np.tile(prob.xf, (B, 1))
    XF[:, 0] += d
    return XF


def cartpole_goals(tog, B, offset=0, XF=None):
    """Config 2 (unconstrained iLQR) with a goal per trajectory in the LQR cost."""
    prob, opts = tog.Problems.config_cartpole(B=B, offset=offset)
    XF = cartpole_goal_set(tog, B, offset) if XF is None else XF
    st, term = prob.obj.stage, prob.obj.terminal
    obj = tog.LQRObjectiveBatch(st.Q, st.R, term.Q, XF, prob.N)
    p = tog.Problem(prob.model, obj, prob._U.copy(), x0=prob.x0.copy(), xf=XF, N=prob.N, dt=prob.dt)
    return p, opts


def cartpole_tracking(tog, B=4):
    """Every trajectory tracks its own reference, on top of the ramped time-varying Hessians with cross terms of
    ramp_objective(cross=0.2): member b keeps knot k's Q_k, R_k, H_k and takes q = -Q_k xr, r = -R_k ur,
    c = 1/2 xr'Q_k xr + 1/2 ur'R_k ur for its reference (xr, ur)(b, k) (per_knot = 1, the dense-cost path)."""
    prob, opts = tog.Problems.config_cartpole(B=B)
    st, term = prob.obj.stage, prob.obj.terminal
    base = ramp_objective(tog, st.Q, st.R, term.Q, prob.xf, prob.N, cross=0.2)
    N, XF = prob.N, cartpole_goal_set(tog, B, offset=100)
    objs = []
    for b in range(B):
        rng = np.random.default_rng(4200 + b)
        costs = []
        for k in range(N - 1):
            s = k / (N - 2)
            xr = s * XF[b] + 0.05 * rng.standard_normal(4)  # a line to the goal, jittered
            ur = 0.1 * rng.standard_normal(1)
            c0 = base[k]
            costs.append(tog.QuadraticCost(c0.Q, c0.R, c0.H, -c0.Q @ xr, -c0.R @ ur,
                                           0.5 * xr @ c0.Q @ xr + 0.5 * ur @ c0.R @ ur))
        objs.append(tog.Objective(costs + [tog.LQRCostTerminal(term.Q, XF[b])]))
    obj = tog.BatchObjective(objs)
    p = tog.Problem(prob.model, obj, prob._U.copy(), x0=prob.x0.copy(), xf=XF, N=N, dt=prob.dt)
    return p, opts


BULK_B = 2304  # above the runtime's TAIL_ACTIVE = 2048: the multi-trajectory team kernels and k_expand_team
BULK_CHECK = (0, 63, 64, 1151, 1152, 2047, 2048, BULK_B - 1)  # first, a wave boundary, the halves' seam, 2048, last
BULK_ITERS = 6


def bulk_problem(tog):
    p, opts = cartpole_goals(tog, BULK_B)
    opts.iterations = BULK_ITERS
    return p, opts


def batch_slice(tog, prob, lo, hi):
    """Trajectories [lo, hi) of a cartpole_goals problem as a batch of their own."""
    st, term = prob.obj.stage, prob.obj.terminal
    obj = tog.LQRObjectiveBatch(st.Q, st.R, term.Q, prob.xf[lo:hi], prob.N)
    p = tog.Problem(prob.model, obj, prob._U[lo:hi].copy(), x0=prob.x0[lo:hi].copy(), xf=prob.xf[lo:hi], N=prob.N,
                    dt=prob.dt)
    return p


_ORACLE = {}


def oracle_solve(oracle, key, prob, opts, trajs=None):
    """Per-trajectory oracle results of prob (computed once per key, shared, never modified):
    {b: (X, U, steps, stats)} with the oracle run on prob.trajectory(b)."""
    if key not in _ORACLE:
        out = {}
        for b in (range(prob.B) if trajs is None else trajs):
            o = oracle.OracleSolver(prob.trajectory(b), opts, b=0)
            steps = o.solve()
            X, U, st = o.get("X"), o.get("U"), o.get("stats")
            for a in (X, U, st):
                a.setflags(write=False)
            out[b] = (X, U, steps, st)
        _ORACLE[key] = out
    return _ORACLE[key]


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def solve_and_compare(tog, oracle, key, prob, opts, env=None, trajs=None):
    gp = prob.copy()
    solver = with_env(env or {}, lambda: tog.solve_b(gp, opts))
    ref = oracle_solve(oracle, key, prob, opts, trajs)
    J = solver.stats["cost"]
    for b, (X, U, steps, st) in ref.items():
        eX, eU = rel(gp._X[b], X), rel(gp._U[b], U)
        Jo = float(st[tog.abi.STAT_J])
        eJ = abs(J[b] - Jo) / max(1.0, abs(Jo))
        print(f"traj {b}: errX {eX:.3e} errU {eU:.3e} errJ {eJ:.3e} steps {int(solver.stats['iterations_total'][b])}"
              f" / {steps}")
        assert eX < TOL_SOLVE and eU < TOL_SOLVE, b
        assert steps == int(solver.stats["iterations_total"][b]), b
        assert eJ < TOL_J, b
    return gp, solver


# ----------------------------------------------------------------------------- CPU: host layer


def test_batch_objective_tables(tog):
    """lin (B, n+m+1) rows [q; r; c] (one stage cost per member) or (B, N-1, n+m+1) (a member with per-knot
    costs), term (B, n+1) rows [qf; cf]; [b] is the member; the Objective face is trajectory 0's."""
    n, m, N, B = 3, 2, 6, 4
    rng = np.random.default_rng(0)
    Q, R, Qf = np.diag([1.0, 2.0, 3.0]), np.diag([0.5, 0.25]), 10.0 * np.eye(n)
    XF = rng.standard_normal((B, n))
    obj = tog.LQRObjectiveBatch(Q, R, Qf, XF, N)
    assert obj.B == B and len(obj) == N and not obj.per_knot
    assert obj.lin.shape == (B, n + m + 1) and obj.term.shape == (B, n + 1)
    for b in range(B):
        c, t = obj[b].stage, obj[b].terminal
        assert np.array_equal(obj.lin[b], np.concatenate([c.q, c.r, [c.c]]))
        assert np.array_equal(obj.term[b], np.concatenate([t.q, [t.c]]))
    assert obj.stage is obj[0].stage and obj.terminal is obj[0].terminal and obj.stage_table(m) is None
    # per-knot members
    objs = []
    for b in range(B):
        costs = [tog.QuadraticCost(Q, R, None, rng.standard_normal(n), rng.standard_normal(m), float(b + k))
                 for k in range(N - 1)]
        objs.append(tog.Objective(costs + [tog.LQRCostTerminal(Qf, XF[b])]))
    ob = tog.BatchObjective(objs)
    assert ob.per_knot and ob.lin.shape == (B, N - 1, n + m + 1)
    for b in range(B):
        for k in range(N - 1):
            c = objs[b][k]
            assert np.array_equal(ob.lin[b, k], np.concatenate([c.q, c.r, [c.c]]))


def test_trajectory_round_trip_is_bitwise(tog):
    """LQRObjectiveBatch(...)[b] is LQRObjective(Q, R, Qf, XF[b], N) bit for bit, and Problem.trajectory(b) is
    the plain B = 1 problem of b: objective, goal constraint, xf, x0, U, X; copy() keeps the data."""
    prob, _ = tog.Problems.config_quadrotor_goals(B=5)
    st, term = prob.obj.stage, prob.obj.terminal
    assert prob.has_trajectory_data() and prob.copy().has_trajectory_data()
    assert prob.copy().obj is prob.obj and np.array_equal(prob.copy().trajectory_goals(), prob.xf)
    prob._X[...] = np.random.default_rng(1).standard_normal(prob._X.shape)
    for b in range(prob.B):
        one = tog.LQRObjective(st.Q, st.R, term.Q, prob.xf[b], prob.N)
        for f in ("Q", "R", "H", "q", "r"):
            assert np.array_equal(getattr(prob.obj[b].stage, f), getattr(one.stage, f))
        assert prob.obj[b].stage.c == one.stage.c
        assert np.array_equal(prob.obj[b].terminal.q, one.terminal.q) and prob.obj[b].terminal.c == one.terminal.c
        t = prob.trajectory(b)
        assert t.B == 1 and not t.batched and not t.has_trajectory_data()
        assert t.obj is prob.obj[b] and np.array_equal(t.xf, prob.xf[b])
        assert np.array_equal(t.x0[0], prob.x0[b]) and np.array_equal(t._U[0], prob._U[b])
        assert np.array_equal(t._X[0], prob._X[b])
        goal = [c for c in t.constraints[prob.N - 1] if isinstance(c, tog.GoalConstraint)]
        assert len(goal) == 1 and np.array_equal(goal[0].xf, prob.xf[b])
        d = t.build_desc().desc
        assert d.batch == 1 and np.array_equal(np.ctypeslib.as_array(d.q, (13,)), one.stage.q)


def test_max_violation_honours_each_goal(tog):
    prob, _ = tog.Problems.config_quadrotor_goals(B=3)
    prob._X[...] = 0.0
    prob._U[...] = 1.0  # inside the control bounds
    for b in range(3):
        prob._X[b, -1] = prob.xf[b]
    prob._X[1, -1, 2] += 0.25
    assert np.array_equal(tog.max_violation(prob), [0.0, 0.25, 0.0])


def test_error_paths_on_the_host(tog):
    n, m, N = 3, 2, 5
    Q, R, Qf = np.eye(n), np.eye(m), np.eye(n)
    a = tog.LQRObjective(Q, R, Qf, np.zeros(n), N)
    costs = list(a.cost)
    costs[2] = tog.LQRCost(2.0 * Q, R, np.zeros(n))
    with pytest.raises(ValueError, match=r"trajectory 1, knot 2"):
        tog.BatchObjective([a, tog.Objective(costs)])
    with pytest.raises(ValueError, match=r"trajectory 1, knot 4"):
        tog.BatchObjective([a, tog.LQRObjective(Q, R, 3.0 * Qf, np.zeros(n), N)])
    with pytest.raises(ValueError):
        tog.LQRObjectiveBatch(Q, R, Qf, np.zeros(n), N)  # XF must be (B, n)
    prob, opts = tog.Problems.config_quadrotor_goals(B=3)
    with pytest.raises(ValueError, match="3 objectives, the problem 2 trajectories"):  # wrong shapes against the batch
        tog.Problem(prob.model, prob.obj, x0=prob.x0[:2], N=prob.N, dt=prob.dt)
    with pytest.raises(ValueError, match=r"\(B, n\)"):
        tog.Problem(prob.model, prob.obj[0], x0=prob.x0, xf=prob.xf[:2], N=prob.N, dt=prob.dt)
    cons = tog.Constraints(prob.N)
    cons[prob.N - 1] += tog.goal_constraint(prob.xf[:2])
    with pytest.raises(ValueError, match="2 goals"):
        tog.Problem(prob.model, prob.obj[0], constraints=cons, x0=prob.x0, N=prob.N, dt=prob.dt)
    # ALTRO and projected Newton refuse before any device call (this test runs without a device)
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.solve_b(prob.copy(), tog.ALTROSolverOptions(opts_al=opts))
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.solve_b(prob.copy(), tog.ProjectedNewtonSolverOptions())
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.ProjectedNewtonSolver(prob.copy())
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.AbstractSolverFor(prob.copy(), tog.ALTROSolverOptions(opts_al=opts))


def test_abi_mirrors(tog):
    """TOG_ABI_VERSION 5 and both entry points in the header, abi.py and libtog.jl."""
    hdr = (ROOT / "include" / "tog.h").read_text()
    jl = (ROOT / "integration" / "julia" / "libtog.jl").read_text()
    assert "#define TOG_ABI_VERSION 5" in hdr and tog.abi.TOG_ABI_VERSION == 5
    assert "TOG_ABI_VERSION = Int32(5)" in jl
    for name in ("tog_set_trajectory_costs", "tog_set_trajectory_goals"):
        assert name in hdr and name in jl and name in tog.abi.EXPORTED_SYMBOLS


def test_host_tables_under_sanitizers(tmp_path):
    """The new host code of the runtime (csrc/tog_traj_tables.hpp: the split over the parts of a multi handle,
    the goal table, the replace order new-before-old, the argument checks) in a stand-alone program of its own
    under AddressSanitizer + UBSan (tests/c/traj_tables_host.cpp; no device code, no GPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "traj_tables_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "traj_tables_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ----------------------------------------------------------------------------- CPU: the inputs, oracle alone

EXCEPTION_FLAGS = ("TRAJ_COST_BLOWUP", "TRAJ_MAX_REG", "TRAJ_SQRT_PD_FAIL", "TRAJ_SINGULAR", "TRAJ_BP_ABORTED")


def _flags(tog, st):
    f = int(st[tog.abi.STAT_FLAGS])
    exc = sum(getattr(tog.abi, n) for n in EXCEPTION_FLAGS)
    return f, f & exc


def _input_sets(tog):
    sets = []
    for sqrt in (False, True):
        p, o = cartpole_goals(tog, 5)
        o.square_root = sqrt
        sets.append((("cartpole5", sqrt), p, o, None, True))
        p, o = cartpole_tracking(tog, 4)
        o.square_root = sqrt
        sets.append((("tracking4", sqrt), p, o, None, True))
    p, o = tog.Problems.config_quadrotor_goals(B=5)
    sets.append((("quad5",), p, o, None, True))
    p, o = bulk_problem(tog)
    sets.append((("bulk",), p, o, BULK_CHECK, False))  # (iterations capped: held to "no exception" only)
    return sets


def test_inputs_converge_in_the_oracle(tog, oracle):
    """For every goal set a GPU test below uses, each trajectory's oracle solve ends CONVERGED (AL_CONVERGED for
    the AL solve) within the options' iteration limits with no exception flag. The bulk set runs under a capped
    iteration count (its test compares bits, not convergence), so its eight oracle-checked trajectories are held
    to the absence of exception flags."""
    for key, p, o, trajs, must_converge in _input_sets(tog):
        ref = oracle_solve(oracle, key, p, o, trajs)
        for b, (X, U, steps, st) in ref.items():
            f, exc = _flags(tog, st)
            assert exc == 0, (key, b, f)
            assert np.isfinite(X).all() and np.isfinite(U).all(), (key, b)
            if must_converge:
                want = tog.abi.TRAJ_AL_CONVERGED if key[0] == "quad5" else tog.abi.TRAJ_CONVERGED
                assert f & want, (key, b, f)
                assert not f & (tog.abi.TRAJ_MAX_ITERS if key[0] != "quad5" else tog.abi.TRAJ_AL_MAX_ITERS), (key, b, f)


# ----------------------------------------------------------------------------- GPU

ENVS = {"default": {}, "team": {"TOG_BWD_TAIL": "team"}, "full": {"TOG_NO_COMPACT": "1"}, "lds": {"TOG_BWD": "lds"}}


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
@pytest.mark.parametrize("kernels", list(ENVS))
def test_gpu_cartpole_ilqr_goals(tog, oracle, gpu, sqrt, kernels):
    """1. Cartpole iLQR, B = 5 (with four teams to a wave, five trajectories fill one wave of teams and leave a
    partial one), a goal per trajectory, on the default kernels, the one-wave team tail kernel, uncompacted
    launches and the LDS backward kernel."""
    prob, opts = cartpole_goals(tog, 5)
    opts.square_root = sqrt
    solve_and_compare(tog, oracle, ("cartpole5", sqrt), prob, opts, ENVS[kernels])


@pytest.mark.gpu
def test_gpu_quadrotor_al_goals(tog, oracle, gpu):
    """2. Quadrotor AL, goal + bounds, square root, B = 5: the cost's goal and the goal constraint's rows both
    differ per trajectory; c_max below the tolerance for every trajectory against its own goal."""
    prob, opts = tog.Problems.config_quadrotor_goals(B=5)
    gp, solver = solve_and_compare(tog, oracle, ("quad5",), prob, opts)
    assert np.all(solver.stats["c_max"] < opts.constraint_tolerance)
    assert np.all(tog.max_violation(gp) < opts.constraint_tolerance)  # (host side, each against its own goal)
    # the goals differ, and so do the end points
    assert np.max(np.abs(gp._X[:, -1, :3] - prob.xf[:, :3])) < opts.constraint_tolerance
    assert np.min(np.linalg.norm(prob.xf[1:, :3] - prob.xf[0, :3], axis=1)) > 10 * opts.constraint_tolerance


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
def test_gpu_cartpole_tracking_per_knot(tog, oracle, gpu, sqrt):
    """3. Cartpole, B = 4, per_knot = 1: every trajectory tracks its own reference on top of the ramped
    time-varying Hessians with cross terms (both tables, the dense-cost path)."""
    prob, opts = cartpole_tracking(tog, 4)
    assert prob.obj.per_knot and prob.obj.stage_table(1) is not None
    opts.square_root = sqrt
    solve_and_compare(tog, oracle, ("tracking4", sqrt), prob, opts)


@pytest.mark.gpu
def test_gpu_step_level(tog, oracle, gpu):
    """4. Step level, B = 5, random X, U: tog_cost (al 0 and 1), TOG_FIELD_C after tog_update_constraints and
    TOG_FIELD_Q after tog_cost_expansion, each trajectory against the oracle on its own problem. Bit for bit, as
    tests/test_cost_expansion.py holds the shared objective (the arithmetic contract: same operations, same
    order; only where q, r, c, qf, cf and the goal come from differs)."""
    prob, opts = tog.Problems.config_quadrotor_goals(B=5)
    rng = np.random.default_rng(7)
    prob._X[...] = rng.standard_normal(prob._X.shape)
    prob._U[...] = tog.Problems.HOVER + rng.standard_normal(prob._U.shape)
    h = tog.AugmentedLagrangianSolver(prob, opts).handle
    J0, J1 = h.cost(al=False), h.cost(al=True)
    h.update_constraints()
    Cd = h.get(tog.abi.FIELD_C)
    Qd = {}
    for sq in (False, True):
        h.cost_expansion(sqrt=sq, al=True)
        Qd[sq] = h.get(tog.abi.FIELD_Q)
    for b in range(prob.B):
        o = oracle.OracleSolver(prob.trajectory(b), opts, b=0)
        j0, j1 = o.cost(False), o.cost(True)
        print(f"traj {b}: J {J0[b]!r} / {j0!r}  J_al {J1[b]!r} / {j1!r}")
        assert J0[b] == j0 and J1[b] == j1, b
        o.update_constraints()
        assert np.array_equal(Cd[b], o.get("C")), b
        for sq in (False, True):
            assert o.cost_expansion(sq, True) == 0
            assert np.array_equal(Qd[sq][b], o.get("Q")), (b, sq)
    # the same X, U cost differently per trajectory (the tables are read per trajectory)
    assert len(set(J0.tolist())) == prob.B


@pytest.mark.gpu
def test_gpu_bulk_kernels(tog, oracle, gpu):
    """5. config_cartpole(B = 2304) with per-trajectory goals, iterations capped: above TAIL_ACTIVE = 2048, so the
    multi-trajectory team kernels and k_expand_team run. Bitwise equal to the same trajectories solved as two
    batches of 1152 (which take the tail kernels that tests 1-3 pin); eight trajectories against the oracle."""
    prob, opts = bulk_problem(tog)
    gp, solver = solve_and_compare(tog, oracle, ("bulk",), prob, opts, trajs=BULK_CHECK)
    S = solver.handle.get(tog.abi.FIELD_STATS)
    half = BULK_B // 2
    for lo in (0, half):
        p = batch_slice(tog, prob, lo, lo + half)
        s = tog.solve_b(p, opts)
        assert np.array_equal(p._X, gp._X[lo:lo + half]) and np.array_equal(p._U, gp._U[lo:lo + half]), lo
        assert np.array_equal(s.handle.get(tog.abi.FIELD_STATS), S[lo:lo + half]), lo


@pytest.mark.gpu
def test_gpu_equal_goals_equal_shared_objective(tog, gpu):
    """6. B = 4 with every row equal to prob.xf: X, U and FIELD_STATS are bitwise the plain problem's."""
    plain, opts = tog.Problems.config_quadrotor(B=4)
    same, _ = tog.Problems.config_quadrotor_goals(B=4)
    XF = np.tile(plain.xf, (4, 1))
    st, term = plain.obj.stage, plain.obj.terminal
    same.obj = tog.LQRObjectiveBatch(st.Q, st.R, term.Q, XF, plain.N)
    same.xf = XF
    for k in range(same.N):
        same.constraints[k] = [tog.goal_constraint(XF) if isinstance(c, tog.GoalConstraint) else c
                               for c in same.constraints[k]]
    assert same.has_trajectory_data() and np.array_equal(same.trajectory_goals(), XF)
    a, b = plain.copy(), same.copy()
    sa, sb = tog.solve_b(a, opts), tog.solve_b(b, opts)
    assert np.array_equal(a._X, b._X) and np.array_equal(a._U, b._U)
    assert np.array_equal(sa.handle.get(tog.abi.FIELD_STATS), sb.handle.get(tog.abi.FIELD_STATS))


def _handle_solve(tog, h, prob, mode):
    """tog_set_state, tog_solve_init + steps to completion (tog_solve), X, U, stats"""
    h.solve(mode)
    return h.get(tog.abi.FIELD_X), h.get(tog.abi.FIELD_U), h.get(tog.abi.FIELD_STATS)


@pytest.mark.gpu
def test_gpu_retargeting(tog, gpu):
    """7. Solve, set new goals and costs on the same handle, solve again: bitwise a fresh handle's result.
    NULL tables return to the shared result."""
    first, opts = tog.Problems.config_quadrotor_goals(B=4)
    second, _ = tog.Problems.config_quadrotor_goals(B=4, offset=50)
    plain, _ = tog.Problems.config_quadrotor(B=4)
    second.x0, second._U = first.x0.copy(), first._U.copy()  # same starts: only the targets change
    opts.iterations = 3
    fresh = second.copy()
    sf = tog.solve_b(fresh, opts)
    Sf = sf.handle.get(tog.abi.FIELD_STATS)
    solver = tog.AugmentedLagrangianSolver(first, opts)
    h = solver.handle
    _handle_solve(tog, h, first, solver.mode)
    h.upload_state(first)  # x0, U, X = NaN again
    h.set_trajectory_costs(second.obj.lin, second.obj.term)
    h.set_trajectory_goals(second.trajectory_goals())
    X, U, S = _handle_solve(tog, h, second, solver.mode)
    assert np.array_equal(X, fresh._X) and np.array_equal(U, fresh._U) and np.array_equal(S, Sf)
    assert not np.array_equal(first.xf, second.xf)
    # back to the shared objective and the descriptor's goal
    shared = plain.copy()
    shared.x0, shared._U = first.x0.copy(), first._U.copy()
    # (the handle's descriptor is trajectory 0 of `first`: the shared problem is that one for every trajectory)
    shared.obj = first.obj[0]
    shared.xf = first.xf[0].copy()
    for k in range(shared.N):
        shared.constraints[k] = [tog.goal_constraint(first.xf[0]) if isinstance(c, tog.GoalConstraint) else c
                                 for c in shared.constraints[k]]
    assert not shared.has_trajectory_data()
    ref = shared.copy()
    ss = tog.solve_b(ref, opts)
    h.upload_state(shared)  # (a problem without per-trajectory data clears the tables: NULL, NULL)
    h.set_trajectory_costs(None, None)
    h.set_trajectory_goals(None)
    X, U, S = _handle_solve(tog, h, shared, solver.mode)
    assert np.array_equal(X, ref._X) and np.array_equal(U, ref._U)
    assert np.array_equal(S, ss.handle.get(tog.abi.FIELD_STATS))


@pytest.mark.gpu
def test_gpu_multi_handle_slices(tog, gpu):
    """8. tog_create_multi over devices [0, 0], B = 5: the slices of 3 and 2 receive their own rows."""
    prob, opts = tog.Problems.config_quadrotor_goals(B=5)
    opts.iterations = 3
    one = prob.copy()
    s1 = tog.solve_b(one, opts)
    two = prob.copy()
    sm = tog.AugmentedLagrangianSolver(two, opts, devices=[0, 0])
    tog.solve_b(two, sm)
    assert np.array_equal(one._X, two._X) and np.array_equal(one._U, two._U)
    assert np.array_equal(s1.handle.get(tog.abi.FIELD_STATS), sm.handle.get(tog.abi.FIELD_STATS))


@pytest.mark.gpu
def test_gpu_refusals(tog, gpu):
    """9. tog_solve_pn with tables set, and the setters on an infeasible and a minimum-time handle, return
    TOG_ERR_UNSUPPORTED with a message; tog_set_trajectory_goals without a goal row returns TOG_ERR_ARG."""
    from test_minimum_time import pendulum_case

    lib = gpu
    ERR_ARG, ERR_UNSUPPORTED = -1, -4
    null = C.cast(None, C.POINTER(C.c_double))
    prob, opts = tog.Problems.config_quadrotor_goals(B=2)
    h = tog.AugmentedLagrangianSolver(prob, opts).handle
    out = np.zeros((2, tog.abi.PN_NSTATS))
    pn = tog.to_tog_pn_options(tog.ProjectedNewtonSolverOptions())
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == ERR_UNSUPPORTED
    assert b"per-trajectory" in lib.tog_last_error()
    h.set_trajectory_costs(None, None)
    h.set_trajectory_goals(None)  # cleared: projected Newton runs again
    h.solve(tog.abi.MODE_AL)
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == 0
    # infeasible start and minimum time
    make, aopts, xf, U0, dt, dt_mt, _ = pendulum_case(tog)
    p = make(U0, dt)
    p.X = tog.line_trajectory([0.0, 0.0], list(xf), p.N)
    for q in (tog.infeasible_problem(p, 1.0), tog.minimum_time_problem(make(U0, dt_mt, tf="min"), 15.0, 0.15, 1e-3)):
        hq = tog.AugmentedLagrangianSolver(q, aopts.opts_al).handle
        lin = np.zeros((1, hq.n + hq.m + 1))
        assert lib.tog_set_trajectory_costs(hq.h, 0, tog.abi.as_dp(lin), null) == ERR_UNSUPPORTED
        assert b"shared" in lib.tog_last_error()
        assert lib.tog_set_trajectory_goals(hq.h, tog.abi.as_dp(np.zeros((1, hq.n)))) == ERR_UNSUPPORTED
    # no goal constraint
    pc, oc = cartpole_goals(tog, 2)
    hc = tog.iLQRSolver(pc, oc).handle
    assert lib.tog_set_trajectory_goals(hc.h, tog.abi.as_dp(np.zeros((2, 4)))) == ERR_ARG
    assert b"no goal constraint" in lib.tog_last_error()
    with pytest.raises(ValueError):
        hc.set_trajectory_costs(np.zeros((3, 6)), None)  # wrong shape: refused on the host
    assert lib.tog_set_trajectory_costs(hc.h, 2, null, null) == ERR_ARG  # per_knot must be 0 or 1
