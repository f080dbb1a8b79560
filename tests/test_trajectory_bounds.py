"""Per-trajectory bounds within one batch (tog_set_trajectory_bounds).

The batch shares which bounds have a row; trajectory b has its own limits (DevProblem::bnd, a (nb, B) table read by
traj_row in csrc/tog_device.hpp at the row's ordinal, which the row keeps in ConRow::b). The oracle solves one
trajectory per descriptor, so trajectory b of such a batch is held to the oracle run on ``prob.trajectory(b)``, the
plain problem of b: X, U within 1e-6 relative, equal iteration counts and STAT_J within 1e-6 relative (TOL_SOLVE and
the step contract of tests/test_trajectory_goals.py); step-level quantities bit for bit, because the arithmetic is
the shared problem's and only where a row's limit comes from differs.

Bound sets (seeds frozen): set A, the car of Problems.car_obstacles in the three-set arrangement (knot 0 a u-only
bound, the stage knots a bound with x and u rows and one infinite entry trimmed, the terminal knot the stage object
and the goal), every limit of every trajectory its own; set B, the quadrotor of config 3 with its thrust limits per
trajectory (the 4-lane k_expand_u path). The CPU test ``test_inputs_converge_in_the_oracle`` holds the inputs
themselves to the conditions that every trajectory's oracle solve ends AL_CONVERGED with no exception flag and that
at least one trajectory per set ends with a bound row at its limit (|c| below the constraint tolerance): bounds
that never bind would let a kernel that ignores the table pass.
"""
import ctypes as C
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
TOL_SOLVE = 1e-6
TOL_J = 1e-6


def rel(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    scale = max(1.0, float(np.max(np.abs(b)))) if b.size else 1.0
    return float(np.max(np.abs(a - b))) / scale if b.size else 0.0


# ----------------------------------------------------------------------------- problems


def car_bounds(tog, B, offset=0, jitter=True, trim=True):
    """Set A: the car of Problems.car_obstacles (its two circles stay the batch's) with U0 = 1 + 0.05 N(0,1) and
    three constraint sets: knot 0 holds a u-only bound (u_min), the stage knots a bound with x and u rows (the
    heading unbounded: trimmed), the terminal knot the stage bound object (its x rows) and the goal. Per trajectory
    (default_rng(8000 + offset + b), drawn in the order U0, d (10,)): knot 0's u_min = [0.1, -2] + 0.05 d[0:2]; the
    stage x_max = [0.5, 1.01] + 0.02 |d[2:4]|, x_min = [-0.5, -0.01] - 0.02 |d[4:6]|, u_max = 1.5 + 0.2 d[6:8],
    u_min = [0.1, -2] + 0.05 d[8:10], d ~ U(-1, 1). jitter = False keeps the problem's own limits in every
    trajectory (the table equals the descriptor's data); trim = False keeps the heading rows with a limit of
    +-(4 + |d|) instead of dropping them."""
    N, n, m = 51, 3, 2
    U0, d = [], []
    for b in range(B):
        r = np.random.default_rng(8000 + offset + b)
        U0.append(1.0 + 0.05 * r.standard_normal((N - 1, m)))
        d.append(r.uniform(-1.0, 1.0, 10) if jitter else np.zeros(10))
    d = np.array(d)
    prob = tog.Problems.car_obstacles(U0=np.stack(U0))
    inf = np.full((B, 1), np.inf) if trim else 4.0 + np.abs(d[:, 0:1])
    bnd1 = tog.BoundConstraint(n, m, u_min=np.array([0.1, -2.0]) + 0.05 * d[:, 0:2], trim=trim)
    bnd = tog.BoundConstraint(
        n, m, trim=trim,
        x_max=np.hstack([np.array([0.5, 1.01]) + 0.02 * np.abs(d[:, 2:4]), inf]),
        x_min=np.hstack([np.array([-0.5, -0.01]) - 0.02 * np.abs(d[:, 4:6]), -inf]),
        u_max=1.5 + 0.2 * d[:, 6:8], u_min=np.array([0.1, -2.0]) + 0.05 * d[:, 8:10])
    cons = tog.Constraints(N)
    cons[0] += bnd1
    for k in range(1, N - 1):
        cons[k] += bnd
        for c in prob.constraints[k]:
            if isinstance(c, tog.CircleConstraints):
                cons[k] += c
    cons[N - 1] += bnd
    cons[N - 1] += tog.goal_constraint(prob.xf)
    out = tog.Problem(prob.model, prob.obj, constraints=cons, x0=prob.x0, xf=prob.xf, N=N, dt=prob.dt)
    out._U[...] = prob._U
    return out, tog.AugmentedLagrangianSolverOptions()


QUAD_MEMBERS = (0, 1, 2, 3, 4)  # of config_quadrotor_bounds(B = 8); member 5 takes 1131 steps in the oracle


def quad_bounds(tog):
    """Set B: config_quadrotor_bounds(B = 8)'s members 0..4: config 3 (goal + control bounds, square root) with the
    thrust limits of each trajectory its own, u_max ~ U(4, 10), u_min ~ U(0, 1)."""
    prob, opts = tog.Problems.config_quadrotor_bounds(B=8)
    return prob.batch_slice(QUAD_MEMBERS[0], QUAD_MEMBERS[-1] + 1), opts


BULK_B = 2304  # above the runtime's TAIL_ACTIVE = 2048: the multi-trajectory team kernels and k_al_outer in bulk
BULK_CHECK = (0, 63, 64, 1151, 1152, 2047, 2048, BULK_B - 1)  # first, a wave boundary, the halves' seam, 2048, last


def bulk_problem(tog):
    p, opts = car_bounds(tog, BULK_B)
    opts.opts_uncon.iterations = 3
    opts.iterations = 2
    return p, opts


_ORACLE = {}


def oracle_solve(oracle, key, prob, opts, trajs=None):
    """Per-trajectory oracle results of prob (computed once per key, shared, never modified):
    {b: (X, U, steps, stats, C)} with the oracle run on prob.trajectory(b); C the constraint values at the result."""
    if key not in _ORACLE:
        out = {}
        for b in (range(prob.B) if trajs is None else trajs):
            o = oracle.OracleSolver(prob.trajectory(b), opts, b=0)
            steps = o.solve()
            X, U, st = o.get("X"), o.get("U"), o.get("stats")
            o.update_constraints()
            Cv = o.get("C")
            for a in (X, U, st, Cv):
                a.setflags(write=False)
            out[b] = (X, U, steps, st, Cv)
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
    for b, (X, U, steps, st, _) in ref.items():
        eX, eU = rel(gp._X[b], X), rel(gp._U[b], U)
        Jo = float(st[tog.abi.STAT_J])
        eJ = abs(J[b] - Jo) / max(1.0, abs(Jo))
        print(f"traj {b}: errX {eX:.3e} errU {eU:.3e} errJ {eJ:.3e} steps {int(solver.stats['iterations_total'][b])}"
              f" / {steps} flags {int(solver.stats['flags'][b]):#x} / {int(st[tog.abi.STAT_FLAGS]):#x}")
        assert eX < TOL_SOLVE and eU < TOL_SOLVE, b
        assert steps == int(solver.stats["iterations_total"][b]), b
        assert int(st[tog.abi.STAT_FLAGS]) == int(solver.stats["flags"][b]), b
        assert eJ < TOL_J, b
    return gp, solver


# ----------------------------------------------------------------------------- CPU: host layer


def test_shapes_and_for_traj(tog):
    """Vectors are the shared constraint, (B, n) / (B, m) arrays hold the limits of each trajectory: batched,
    for_traj(b) is the plain constraint of b, slice keeps a range, to_abi carries trajectory 0's data, length counts
    the kept rows; under trim the finite entries must be the same in every trajectory."""
    rng = np.random.default_rng(0)
    n, m, B = 3, 2, 4
    c1 = tog.BoundConstraint(n, m, u_min=-1.0, u_max=[1.0, 2.0])
    assert not c1.batched and c1.for_traj(3) is c1 and c1.slice(1, 3) is c1 and c1.length() == 4
    um = 1.0 + rng.uniform(0, 1, (B, m))
    xm = np.hstack([rng.uniform(1, 2, (B, 2)), np.full((B, 1), np.inf)])
    cb = tog.BoundConstraint(n, m, u_max=um, u_min=-2.0, x_max=xm)  # (one batched argument batches all four)
    assert cb.batched and cb.length() == 6 and cb.length("terminal") == 2
    assert cb.u_min.shape == (B, m) and cb.x_min.shape == (B, n) and np.all(cb.u_min == -2.0)
    for b in range(B):
        t = cb.for_traj(b)
        assert type(t) is tog.BoundConstraint and not t.batched and t.trim
        assert np.array_equal(t.u_max, um[b]) and np.array_equal(t.x_max, xm[b])
        assert np.array_equal(t.u_min, [-2.0, -2.0]) and np.all(t.x_min == -np.inf)
        assert t.length() == 6 and t.active["x_max"].tolist() == [True, True, False]
    s = cb.slice(1, 3)
    assert s.batched and np.array_equal(s.u_max, um[1:3]) and np.array_equal(s.x_max, xm[1:3])
    kind, count, flat = cb.to_abi(m)
    assert kind == tog.abi.CON_BOUND and count == 0
    assert np.array_equal(flat, cb.for_traj(0).to_abi(m)[2])
    x, u = np.array([0.3, -0.2, 0.1]), np.array([0.5, 2.5])
    assert np.array_equal(cb.evaluate(x, u), cb.for_traj(0).evaluate(x, u))
    assert np.array_equal(cb.evaluate(x), cb.for_traj(0).evaluate(x))
    R = cb.bound_rows(B)
    assert R.shape == (B, 6) and np.array_equal(R[:, 0:2], xm[:, 0:2]) and np.array_equal(R[:, 2:4], um)
    assert np.all(R[:, 4:6] == -2.0)
    assert np.array_equal(cb.bound_rows(B, "terminal"), xm[:, 0:2])
    assert np.array_equal(c1.bound_rows(2), [[1.0, 2.0, -1.0, -1.0]] * 2)
    # the finiteness pattern: trajectory 2's x_max[1] infinite where trajectory 0's is finite
    bad = xm.copy()
    bad[2, 1] = np.inf
    with pytest.raises(ValueError, match=r"x_max\[1\] of trajectory 2"):
        tog.BoundConstraint(n, m, x_max=bad)
    assert tog.BoundConstraint(n, m, x_max=bad, trim=False).length() == 10  # (untrimmed: every row, any pattern)
    with pytest.raises(ValueError, match="trajectory 1"):  # u_max < u_min in one trajectory
        tog.BoundConstraint(n, m, u_max=[[1.0, 1.0], [-3.0, 1.0]], u_min=-2.0)
    with pytest.raises(ValueError, match="one B"):
        tog.BoundConstraint(n, m, u_max=np.ones((3, m)), x_max=np.ones((4, n)))


def test_trajectory_round_trip_is_bitwise(tog):
    """Problem.trajectory(b) is the plain B = 1 problem of b: its limits, x0, U, X, bit for bit, one plain object
    per batched one (knots that share a set keep sharing it, and the terminal knot keeps the stage object);
    copy() keeps the data; batch_slice keeps a range."""
    prob, _ = car_bounds(tog, 6)
    assert prob.has_trajectory_data() and prob.has_trajectory_bounds() and prob.copy().has_trajectory_bounds()
    assert not prob.has_trajectory_obstacles()
    T = prob.trajectory_bounds()
    assert T.shape == (6, 2 + 8 + 4) and np.array_equal(prob.copy().trajectory_bounds(), T)
    plain = tog.Problems.car_obstacles()
    assert not plain.has_trajectory_bounds() and plain.trajectory_bounds() is None
    prob._X[...] = np.random.default_rng(1).standard_normal(prob._X.shape)
    bnd1, bnd = prob.constraints[0][0], prob.constraints[1][0]
    assert prob.constraints[prob.N - 1][0] is bnd
    for b in range(prob.B):
        t = prob.trajectory(b)
        assert t.B == 1 and not t.batched and not t.has_trajectory_data() and t.trajectory_bounds() is None
        assert np.array_equal(t.x0[0], prob.x0[b]) and np.array_equal(t._U[0], prob._U[b])
        assert np.array_equal(t._X[0], prob._X[b])
        t1, ts = t.constraints[0][0], t.constraints[1][0]
        assert not t1.batched and not ts.batched
        assert np.array_equal(t1.u_min, bnd1.u_min[b]) and np.array_equal(ts.x_max, bnd.x_max[b])
        assert np.array_equal(ts.u_max, bnd.u_max[b]) and np.array_equal(ts.x_min, bnd.x_min[b])
        assert t.constraints[2][0] is ts and t.constraints[t.N - 1][0] is ts  # (shared across knots)
        # the table's row of b is the plain problem's descriptor data in row order
        d = t.build_desc()
        assert d.desc.batch == 1 and d.desc.n_sets == 3
        want = np.concatenate([t1.evaluate(np.zeros(3), np.zeros(2)), ts.evaluate(np.zeros(3), np.zeros(2)),
                               ts.evaluate(np.zeros(3))])  # (c at x = u = 0: -a for a max row, +a for a min row)
        sign = np.concatenate([[1, 1], [-1] * 4 + [1] * 4, [-1, -1, 1, 1]])
        assert np.array_equal(T[b], sign * want)
    assert len({T[b].tobytes() for b in range(6)}) == 6
    p = prob.batch_slice(2, 5)
    assert p.B == 3 and p.has_trajectory_bounds() and np.array_equal(p.trajectory_bounds(), T[2:5])
    assert np.array_equal(p.x0, prob.x0[2:5]) and np.array_equal(p._U, prob._U[2:5])
    assert p.constraints[p.N - 1][0] is p.constraints[1][0]
    for b in range(3):
        a, c = p.trajectory(b), prob.trajectory(2 + b)
        assert np.array_equal(a.constraints[1][0].u_max, c.constraints[1][0].u_max)
        assert np.array_equal(a.build_desc().desc.sets[1].con[0].data[0:10], c.build_desc().desc.sets[1].con[0].data[0:10])


def test_trajectory_bounds_order(tog):
    """The ordinal order of the ABI on three sets: knot 0 a u-only bound (2 rows), the stage knots a bound with x
    and u rows and the heading trimmed (x_max 2, u_max 2, x_min 2, u_min 2), the terminal knot the stage object, of
    which only the x rows count (x_max 2, x_min 2). A set used at many knots counts once."""
    B = 3
    prob, _ = car_bounds(tog, B)
    bnd1, bnd = prob.constraints[0][0], prob.constraints[1][0]
    d = prob.build_desc().desc
    assert d.n_sets == 3 and [d.knot_set[k] for k in range(prob.N)] == [0] + [1] * (prob.N - 2) + [2]
    T = prob.trajectory_bounds()
    assert T.shape == (B, 14)
    assert np.array_equal(T[:, 0:2], bnd1.u_min)
    assert np.array_equal(T[:, 2:4], bnd.x_max[:, 0:2]) and np.array_equal(T[:, 4:6], bnd.u_max)
    assert np.array_equal(T[:, 6:8], bnd.x_min[:, 0:2]) and np.array_equal(T[:, 8:10], bnd.u_min)
    assert np.array_equal(T[:, 10:12], bnd.x_max[:, 0:2]) and np.array_equal(T[:, 12:14], bnd.x_min[:, 0:2])
    # shared data beside batched data, and a non-bound constraint between two bounds of one set
    n, m, N = 3, 2, 6
    obj = tog.LQRObjective(np.eye(n), np.eye(m), np.eye(n), np.zeros(n), N)
    model = tog.rk4(tog.Dynamics.car)
    a = tog.BoundConstraint(n, m, u_max=np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]))
    s = tog.BoundConstraint(n, m, x_min=[-9.0, -np.inf, -7.0])
    circ = tog.CircleConstraints(n, m, [[0.0, 0.0, 0.1]])
    cons = tog.Constraints(N)
    for k in range(1, N - 1):
        cons[k] += a
        cons[k] += circ
        cons[k] += s
    p = tog.Problem(model, obj, constraints=cons, x0=np.zeros((B, n)), N=N, dt=0.1)
    T = p.trajectory_bounds()
    assert T.shape == (B, 4) and np.array_equal(T[:, 0:2], a.u_max) and np.all(T[:, 2:4] == [-9.0, -7.0])


def test_untrimmed_constraint(tog):
    """trim = False keeps every row: 2 (n + m) at a stage knot, 2 n at the terminal one, infinite limits included."""
    B = 3
    prob, _ = car_bounds(tog, B, trim=False)
    bnd1, bnd = prob.constraints[0][0], prob.constraints[1][0]
    assert bnd.to_abi(2)[1] == 1 and bnd.length() == 10 and bnd.length("terminal") == 6
    T = prob.trajectory_bounds()
    assert T.shape == (B, 10 + 10 + 6)
    assert np.all(np.isposinf(T[:, 0:5])) and np.all(np.isneginf(T[:, 5:8])) and np.array_equal(T[:, 8:10], bnd1.u_min)
    assert np.array_equal(T[:, 10:13], bnd.x_max) and np.array_equal(T[:, 13:15], bnd.u_max)
    assert np.array_equal(T[:, 15:18], bnd.x_min) and np.array_equal(T[:, 18:20], bnd.u_min)
    assert np.array_equal(T[:, 20:23], bnd.x_max) and np.array_equal(T[:, 23:26], bnd.x_min)
    assert np.array_equal(prob.trajectory(1).constraints[1][0].x_max, bnd.x_max[1])


def test_wrong_batch_raises(tog):
    prob, _ = car_bounds(tog, 3)
    with pytest.raises(ValueError, match="BoundConstraint holds the limits of 3 trajectories, the problem 2"):
        tog.Problem(prob.model, prob.obj, constraints=prob.constraints, x0=prob.x0[:2], N=prob.N, dt=prob.dt)


def test_max_violation_honours_each_limit(tog):
    """Every trajectory against its own limits: trajectory 1's u_max[0] is 1.2; a control of 1.25 lies outside it
    and inside the other trajectories' limits."""
    prob, _ = car_bounds(tog, 3, jitter=False)
    bnd = prob.constraints[1][0]
    um = bnd.u_max.copy()
    um[1, 0] = 1.2
    new = tog.BoundConstraint(3, 2, x_max=bnd.x_max, x_min=bnd.x_min, u_max=um, u_min=bnd.u_min)
    cons = tog.Constraints(prob.N)
    for k in range(prob.N):
        cons[k] = tog.ConstraintSet(new if c is bnd else c for c in prob.constraints[k])
    prob = tog.Problem(prob.model, prob.obj, constraints=cons, x0=prob.x0, xf=prob.xf, N=prob.N, dt=prob.dt)
    prob._X[...] = 0.0
    prob._X[:, :, 0] = -0.3  # (away from both circles)
    prob._U[...] = 1.0
    prob._U[:, 5, 0] = 1.25
    prob._X[:, -1] = prob.xf
    v = tog.max_violation(prob)
    assert v[0] == 0.0 and v[2] == 0.0
    assert v[1] == 1.25 - 1.2


def test_solver_refusals_on_the_host(tog):
    """ALTRO, projected Newton and solve_stream refuse before any device call (this test runs without a device)."""
    prob, opts = car_bounds(tog, 3)
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.solve_b(prob.copy(), tog.ALTROSolverOptions(opts_al=opts))
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.AbstractSolverFor(prob.copy(), tog.ALTROSolverOptions(opts_al=opts))
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.solve_b(prob.copy(), tog.ProjectedNewtonSolverOptions())
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.ProjectedNewtonSolver(prob.copy())
    with pytest.raises(ValueError, match="per-trajectory bounds"):
        tog.solve_stream(prob.copy(), opts, slots=2)


def test_abi_mirrors(tog):
    """The entry point in the header, abi.py and libtog.jl; TOG_ABI_VERSION still 5 (a new function only)."""
    hdr = (ROOT / "include" / "tog.h").read_text()
    jl = (ROOT / "integration" / "julia" / "libtog.jl").read_text()
    assert "#define TOG_ABI_VERSION 5" in hdr and tog.abi.TOG_ABI_VERSION == 5
    assert "TOG_ABI_VERSION = Int32(5)" in jl
    name = "tog_set_trajectory_bounds"
    assert f"int32_t {name}(tog_handle* h, const double* bnd);" in hdr
    assert f"(:{name}, libtog)" in jl and name in tog.abi.EXPORTED_SYMBOLS


def test_host_plan_under_sanitizers(tmp_path):
    """The host plan of the bound table (csrc/tog_traj_tables.hpp: ordinals, nb, the argument checks, the part
    slices, the error texts) in a stand-alone program under AddressSanitizer + UBSan
    (tests/c/traj_bounds_host.cpp; no device code, no GPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "traj_bounds_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "traj_bounds_host.cpp"), "-o", str(exe)],
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


def _bound_row_mask(tog, t):
    """(N, pmax) mask of the bound rows of the plain problem t, in the constraint vector's order"""
    pm = max(t.constraints.num_constraints())
    mask = np.zeros((t.N, pm), bool)
    for k in range(t.N):
        kind = "terminal" if k == t.N - 1 else "stage"
        o = 0
        for c in t.constraints[k]:
            L = c.length(kind)
            if isinstance(c, tog.BoundConstraint):
                mask[k, o:o + L] = True
            o += L
    return mask


def _input_sets(tog):
    sets = []
    for sqrt in (False, True):
        p, o = car_bounds(tog, 5)
        o.opts_uncon.square_root = sqrt
        sets.append((("car5", sqrt), p, o, None, True))
    p, o = quad_bounds(tog)
    sets.append((("quad5",), p, o, None, True))
    p, o = bulk_problem(tog)
    sets.append((("bulk",), p, o, BULK_CHECK, False))  # (iterations capped: held to "no exception" only)
    return sets


def test_inputs_converge_in_the_oracle(tog, oracle):
    """For every bound set a GPU test below uses, each trajectory's oracle solve ends AL_CONVERGED within the
    options' iteration limits with no exception flag and finite X, U, and at least one trajectory of the set ends
    with a bound row at its limit: |c| below the constraint tolerance. The bulk set runs under capped iteration
    counts (its test compares bits, not convergence), so its eight oracle-checked trajectories are held to the
    absence of exception flags."""
    for key, p, o, trajs, must_converge in _input_sets(tog):
        ref = oracle_solve(oracle, key, p, o, trajs)
        binding = 0
        for b, (X, U, steps, st, Cv) in ref.items():
            f, exc = _flags(tog, st)
            mask = _bound_row_mask(tog, p.trajectory(b))
            at_limit = int(np.sum(np.abs(Cv[:, :mask.shape[1]][mask]) < o.constraint_tolerance))
            binding += at_limit > 0
            print(key, b, steps, hex(f), "bound rows at their limit:", at_limit)
            assert exc == 0, (key, b, f)
            assert np.isfinite(X).all() and np.isfinite(U).all(), (key, b)
            if must_converge:
                assert f & tog.abi.TRAJ_AL_CONVERGED, (key, b, f)
                assert not f & tog.abi.TRAJ_AL_MAX_ITERS, (key, b, f)
        if must_converge:
            assert binding >= 1, key


def test_config_quadrotor_bounds(tog, oracle):
    """Problems.config_quadrotor_bounds: config 3's starts, the documented ranges, and each of the first 8
    trajectories ends AL_CONVERGED in the oracle without an exception flag and with a control-bound row at its
    limit at the solution (members 0..4 are set B's and share its oracle runs; 5..7 are run here)."""
    prob, opts = tog.Problems.config_quadrotor_bounds(B=8)
    base, _ = tog.Problems.config_quadrotor(B=8)
    assert np.array_equal(prob.x0, base.x0) and np.array_equal(prob._U, base._U)
    T = prob.trajectory_bounds()
    assert T.shape == (8, 8)
    lo, hi = tog.Problems.QUAD_BOUNDS_U_MAX
    assert np.all((T[:, 0:4] >= lo) & (T[:, 0:4] <= hi)) and np.all(T[:, 0:4] == T[:, 0:1])
    lo, hi = tog.Problems.QUAD_BOUNDS_U_MIN
    assert np.all((T[:, 4:8] >= lo) & (T[:, 4:8] <= hi)) and np.all(T[:, 4:8] == T[:, 4:5])
    assert len(set(T[:, 0].tolist())) == 8
    q, qo = quad_bounds(tog)
    assert np.array_equal(q.trajectory_bounds(), T[:5])
    ref = list(oracle_solve(oracle, ("quad5",), q, qo).values())
    ref += list(oracle_solve(oracle, ("quad5to7",), prob, opts, trajs=(5, 6, 7)).values())
    assert len(ref) == 8
    for b, (X, U, steps, st, Cv) in enumerate(ref):
        f, exc = _flags(tog, st)
        at_limit = int(np.sum(np.abs(Cv[:prob.N - 1, :8]) < opts.constraint_tolerance))
        print(b, steps, hex(f), "control-bound rows at their limit:", at_limit)
        assert exc == 0 and f & tog.abi.TRAJ_AL_CONVERGED and not f & tog.abi.TRAJ_AL_MAX_ITERS, (b, f)
        assert at_limit > 0, b


def _row_table(tog, prob, with_ordinals):
    """build_rows (csrc/tog_runtime.cpp) restated on the host: the rows of every knot over Problem._abi_sets, a
    bound row as (type, index, limit, ordinal or 0), any other row as (kind, index, data, set index for a circle
    or sphere: its ordinal differs per set), and the de-duplication of knots with equal rows. Returns
    (nrows, knot_off, knot_cnt)."""
    sets, knot_set = prob._abi_sets()
    N = prob.N
    term_set = knot_set[N - 1]
    base, nb = {}, 0
    for s, cs in enumerate(sets):
        for ci, c in enumerate(cs):
            if isinstance(c, tog.BoundConstraint):
                base[(s, ci)] = nb
                nb += c.length("terminal" if s == term_set else "stage")
    rows, off, cnt = [], [], []
    for k in range(N):
        off.append(len(rows))
        s = knot_set[k]
        if s < 0:
            cnt.append(0)
            continue
        term = k == N - 1
        for ci, c in enumerate(sets[s]):
            if isinstance(c, tog.BoundConstraint):
                o = base[(s, ci)]
                for name in (("x_max", "x_min") if term else ("x_max", "u_max", "x_min", "u_min")):
                    v = getattr(c, name)
                    v = v[0] if c.batched else v
                    for i in np.nonzero(c.active[name])[0]:
                        rows.append((name, int(i), float(v[i]), o if with_ordinals else 0))
                        o += 1
            else:
                kind, _, data = c.to_abi(None) if isinstance(c, tog.InfeasibleConstraint) else c.to_abi()
                per_set = s if kind in (tog.abi.CON_CIRCLES, tog.abi.CON_SPHERES) else 0
                for i in range(c.length("terminal" if term else "stage")):
                    rows.append((kind, i, tuple(np.asarray(data).ravel().tolist()), per_set))
        cnt.append(len(rows) - off[k])
        for j in range(k):
            if cnt[j] == cnt[k] and cnt[k] > 0 and rows[off[j]:off[j] + cnt[j]] == rows[off[k]:off[k] + cnt[k]]:
                del rows[off[k]:]
                off[k] = off[j]
                break
    return len(rows), off, cnt


def test_row_table_keeps_its_shape(tog):
    """Storing the ordinal in the bound rows changes nrows, knot_off and knot_cnt for no problem that Problems.*
    builds: none of them has two distinct sets with equal bound rows, the one case in which the de-duplication
    stops sharing a copy. A hand-made problem that has (state bounds alone at the stage knots and, as another set,
    at the terminal knot) shows the restatement sees the difference."""
    P = tog.Problems
    cases = {
        "doubleintegrator": P.doubleintegrator, "cartpole": P.cartpole, "quad_obs": P.quad_obs,
        "quadrotor_test": lambda: P.quadrotor_test("goal+bounds"),
        "quadrotor_test obs": lambda: P.quadrotor_test("goal+bounds+obs"),
        "car_sqrt_bp": lambda: P.car_sqrt_bp(True), "pendulum": P.pendulum, "car_parallel_park": P.car_parallel_park,
        "car_obstacles": P.car_obstacles, "kuka": lambda: P.kuka(U0=np.zeros((50, 7))),
        "quadrotor_maze": P.quadrotor_maze, "quadrotor_maze_batch": lambda: P.quadrotor_maze_batch(2),
        "config_cartpole": lambda: P.config_cartpole(B=2), "config_quadrotor": lambda: P.config_quadrotor(B=2),
        "config_quadrotor_goals": lambda: P.config_quadrotor_goals(B=2),
        "config_quadrotor_tv": lambda: P.config_quadrotor_tv(B=2),
        "config_quadrotor_bounds": lambda: P.config_quadrotor_bounds(B=2),
        "config_quad_maze": lambda: P.config_quad_maze(B=2, N=21),
        "config_quad_maze_obstacles": lambda: P.config_quad_maze_obstacles(B=2, N=21),
        "config_doubleintegrator": P.config_doubleintegrator,
    }
    for name, make in cases.items():
        p = make()
        p = p[0] if isinstance(p, tuple) else p
        assert _row_table(tog, p, False) == _row_table(tog, p, True), name
    n, m, N = 3, 2, 6
    bnd = tog.BoundConstraint(n, m, x_max=[1.0, 2.0, 3.0])
    obj = tog.LQRObjective(np.eye(n), np.eye(m), np.eye(n), np.zeros(n), N)
    p = tog.Problem(tog.rk4(tog.Dynamics.car), obj, constraints=tog.Constraints([bnd], N), x0=np.zeros(n), N=N, dt=0.1)
    assert _row_table(tog, p, False)[0] == 3 and _row_table(tog, p, True)[0] == 6


def test_transforms_refuse(tog):
    """infeasible_problem and minimum_time_problem build their combined bounds from one set of limits: a problem
    with per-trajectory limits is refused with a ValueError naming the transform."""
    prob, _ = car_bounds(tog, 3)
    with pytest.raises(ValueError, match="infeasible_problem: the problem has per-trajectory bounds"):
        tog.infeasible_problem(prob, 1.0)
    with pytest.raises(ValueError, match="minimum_time_problem: the problem has per-trajectory bounds"):
        tog.minimum_time_problem(prob, 15.0, 0.15, 1e-3)


# ----------------------------------------------------------------------------- GPU

ENVS = {"default": {}, "team": {"TOG_BWD_TAIL": "team"}, "full": {"TOG_NO_COMPACT": "1"}, "lds": {"TOG_BWD": "lds"}}


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
@pytest.mark.parametrize("kernels", list(ENVS))
def test_gpu_car_bounds(tog, oracle, gpu, sqrt, kernels):
    """1. Set A, B = 5 (with four teams to a wave, five trajectories fill one wave of teams and leave a partial
    one): state and control bounds in three sets, each trajectory its own limits, on the default kernels, the
    one-wave team tail kernel, uncompacted launches and the LDS backward kernel."""
    prob, opts = car_bounds(tog, 5)
    opts.opts_uncon.square_root = sqrt
    gp, solver = solve_and_compare(tog, oracle, ("car5", sqrt), prob, opts, ENVS[kernels])
    assert np.all(tog.max_violation(gp) < opts.constraint_tolerance)  # (host side, each against its own limits)


@pytest.mark.gpu
def test_gpu_quadrotor_bounds(tog, oracle, gpu):
    """2. Set B: quadrotor AL, control bounds + goal, square root: the stage knots hold control-bound rows only, so
    their expansion runs on k_expand_u's 4-lane teams (row r on lane r % 4, four trajectories and 16 knots to a
    wave). c_max and the host max_violation below the tolerance for every trajectory against its own limits."""
    prob, opts = quad_bounds(tog)
    gp, solver = solve_and_compare(tog, oracle, ("quad5",), prob, opts)
    assert np.all(solver.stats["c_max"] < opts.constraint_tolerance)
    assert np.all(tog.max_violation(gp) < opts.constraint_tolerance)


def _maze_step_problem(tog):
    """config_quad_maze_obstacles(B = 5, N = 11) with per-trajectory limits on all three of its bounds (each finite
    limit moved by U(-0.5, 0.5), the upper ones up and the lower ones down where the two coincide), a goal per
    trajectory beside the terminal bound, and seeded X, U around the limits: the bound table, the obstacle table
    and the goal table on one handle."""
    prob, opts = tog.Problems.config_quad_maze_obstacles(B=5, N=11)
    B, N, n, m = prob.B, prob.N, 13, 4
    rng = np.random.default_rng(21)

    def batched(c):
        lim = {}
        for name, sgn in (("x_max", 1.0), ("u_max", 1.0), ("x_min", -1.0), ("u_min", -1.0)):
            v = np.tile(getattr(c, name), (B, 1))
            fin = np.isfinite(v)
            v[fin] += (sgn * rng.uniform(0.0, 0.5, v.shape))[fin]
            lim[name] = v
        return tog.BoundConstraint(n, m, **lim)

    swap = {}
    for k in (0, 1, N - 1):
        for c in prob.constraints[k]:
            if isinstance(c, tog.BoundConstraint) and id(c) not in swap:
                swap[id(c)] = batched(c)
    XF = np.tile(prob.xf, (B, 1)) + rng.uniform(-1.0, 1.0, (B, n))
    cons = tog.Constraints(N)
    for k in range(N):
        cons[k] = tog.ConstraintSet(swap.get(id(c), c) for c in prob.constraints[k])
    cons[N - 1] += tog.goal_constraint(XF)
    out = tog.Problem(prob.model, prob.obj, constraints=cons, x0=prob.x0, xf=prob.xf, N=N, dt=prob.dt)
    out._X[...] = rng.standard_normal(out._X.shape) * 15.0  # (x limits of +-25, 0..20: rows on both sides)
    out._U[...] = tog.Problems.HOVER + 30.0 * rng.uniform(-1.0, 1.0, out._U.shape)  # (u in 0..50)
    return out, opts


def test_step_inputs_have_active_bound_rows(tog, oracle):
    """The step-level inputs, on the oracle alone: every trajectory has bound rows with c > 0 and with c < 0, and
    the three tables are all there."""
    prob, opts = _maze_step_problem(tog)
    assert prob.has_trajectory_bounds() and prob.has_trajectory_obstacles() and prob.trajectory_goals() is not None
    assert prob.trajectory_bounds().shape == (5, 8 + 12 + 18)  # knot 0: 8 u; stage: 4 x, 8 u; terminal: 18 x
    for b in range(prob.B):
        t = prob.trajectory(b)
        o = oracle.OracleSolver(t, opts, b=0)
        o.update_constraints()
        Co = o.get("C")
        mask = _bound_row_mask(tog, t)
        c = Co[:, :mask.shape[1]][mask]
        assert np.sum(c > 0.0) >= 5 and np.sum(c < 0.0) >= 5, b


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
def test_gpu_step_level(tog, oracle, gpu, sqrt):
    """3. Step level, B = 5, state and control bounds, cylinders, spheres and a goal, with the bound table, the
    obstacle table and the goal table all set on one handle: tog_cost (al 0 and 1), TOG_FIELD_C after
    tog_update_constraints and TOG_FIELD_Q after tog_cost_expansion (std or square root), each trajectory against
    the oracle on its own problem, bit for bit."""
    prob, opts = _maze_step_problem(tog)
    h = tog.AugmentedLagrangianSolver(prob, opts).handle
    assert h._traj_bounds and h._traj_obstacles and h._traj_goals
    J0, J1 = h.cost(al=False), h.cost(al=True)
    h.update_constraints()
    Cd = h.get(tog.abi.FIELD_C)
    h.cost_expansion(sqrt=sqrt, al=True)
    Qd = h.get(tog.abi.FIELD_Q)
    for b in range(prob.B):
        t = prob.trajectory(b)
        o = oracle.OracleSolver(t, opts, b=0)
        j0, j1 = o.cost(False), o.cost(True)
        print(f"traj {b}: J {J0[b]!r} / {j0!r}  J_al {J1[b]!r} / {j1!r}")
        o.update_constraints()
        Co = o.get("C")
        assert J0[b] == j0 and J1[b] == j1, b
        assert np.array_equal(Cd[b], Co), b
        assert o.cost_expansion(sqrt, True) == 0
        assert np.array_equal(Qd[b], o.get("Q")), b
    assert len(set(J1.tolist())) == prob.B


@pytest.mark.gpu
def test_gpu_bulk_kernels(tog, oracle, gpu):
    """4. Set A's generator at B = 2304 with 3 inner and 2 outer iterations: above TAIL_ACTIVE = 2048, so the
    multi-trajectory team kernels, k_expand_team and k_al_outer run in bulk. Bitwise equal to the same trajectories
    solved as two batches of 1152; eight trajectories against the oracle."""
    prob, opts = bulk_problem(tog)
    gp, solver = solve_and_compare(tog, oracle, ("bulk",), prob, opts, trajs=BULK_CHECK)
    S = solver.handle.get(tog.abi.FIELD_STATS)
    half = BULK_B // 2
    for lo in (0, half):
        p = prob.batch_slice(lo, lo + half)
        s = tog.solve_b(p, opts)
        assert np.array_equal(p._X, gp._X[lo:lo + half]) and np.array_equal(p._U, gp._U[lo:lo + half]), lo
        assert np.array_equal(s.handle.get(tog.abi.FIELD_STATS), S[lo:lo + half]), lo


def _shared_car(tog, like):
    """the plain problem whose limits are trajectory 0's of `like`, with like's starts (same three sets)"""
    t0 = like.trajectory(0)
    out = tog.Problem(like.model, like.obj, constraints=t0.constraints, x0=like.x0, xf=like.xf, N=like.N, dt=like.dt)
    out._U[...] = like._U
    return out


@pytest.mark.gpu
def test_gpu_equal_tables_equal_shared_problem(tog, gpu):
    """5. A table of B copies of the descriptor's values: X, U and FIELD_STATS are bitwise the plain problem's."""
    same, opts = car_bounds(tog, 5, jitter=False)
    assert same.has_trajectory_bounds()
    plain = _shared_car(tog, same)
    assert not plain.has_trajectory_data()
    a, b = plain.copy(), same.copy()
    sa, sb = tog.solve_b(a, opts), tog.solve_b(b, opts)
    assert not sa.handle.__dict__.get("_traj_bounds", False) and sb.handle._traj_bounds
    assert np.array_equal(a._X, b._X) and np.array_equal(a._U, b._U)
    assert np.array_equal(sa.handle.get(tog.abi.FIELD_STATS), sb.handle.get(tog.abi.FIELD_STATS))


def _handle_solve(tog, h, mode):
    h.solve(mode)
    return h.get(tog.abi.FIELD_X), h.get(tog.abi.FIELD_U), h.get(tog.abi.FIELD_STATS)


@pytest.mark.gpu
def test_gpu_retargeting(tog, gpu):
    """6. Solve, set another table on the same handle, solve again: bitwise a fresh handle's result. NULL returns
    to the shared result (the descriptor's limits, trajectory 0's, for every trajectory)."""
    first, opts = car_bounds(tog, 5)
    second, _ = car_bounds(tog, 5, offset=50)
    second._U[...] = first._U  # same starts: only the limits change
    assert not np.array_equal(first.trajectory_bounds(), second.trajectory_bounds())
    fresh = second.copy()
    sf = tog.solve_b(fresh, opts)
    Sf = sf.handle.get(tog.abi.FIELD_STATS)
    solver = tog.AugmentedLagrangianSolver(first, opts)
    h = solver.handle
    X1, _, _ = _handle_solve(tog, h, solver.mode)
    h.upload_state(first)  # x0, U, X = NaN again
    h.set_trajectory_bounds(second.trajectory_bounds())
    X, U, S = _handle_solve(tog, h, solver.mode)
    assert np.array_equal(X, fresh._X) and np.array_equal(U, fresh._U) and np.array_equal(S, Sf)
    assert not np.array_equal(X, X1)
    # back to the descriptor's limits: trajectory 0 of `first` for everyone
    shared = _shared_car(tog, first)
    assert not shared.has_trajectory_data()
    ref = shared.copy()
    ss = tog.solve_b(ref, opts)
    h.upload_state(shared)  # (a problem without per-trajectory data clears the table: NULL)
    assert not h._traj_bounds
    X, U, S = _handle_solve(tog, h, solver.mode)
    assert np.array_equal(X, ref._X) and np.array_equal(U, ref._U)
    assert np.array_equal(S, ss.handle.get(tog.abi.FIELD_STATS))


@pytest.mark.gpu
def test_gpu_multi_handle_slices(tog, gpu):
    """7. tog_create_multi over devices [0, 0], B = 5: the slices of 3 and 2 receive their own rows. A table with a
    NaN in the second part's slice is refused whole: the first part keeps its table too."""
    prob, opts = car_bounds(tog, 5)
    one = prob.copy()
    s1 = tog.solve_b(one, opts)
    two = prob.copy()
    sm = tog.AugmentedLagrangianSolver(two, opts, devices=[0, 0])
    tog.solve_b(two, sm)
    assert np.array_equal(one._X, two._X) and np.array_equal(one._U, two._U)
    assert np.array_equal(s1.handle.get(tog.abi.FIELD_STATS), sm.handle.get(tog.abi.FIELD_STATS))
    bad = prob.trajectory_bounds() + 0.01  # (other limits everywhere: a part that took its slice would solve differently)
    bad[4, 0] = np.nan
    assert gpu.tog_set_trajectory_bounds(sm.handle.h, tog.abi.as_dp(bad)) == -1
    assert b"NaN at row 0 of trajectory 4" in gpu.tog_last_error()
    null = C.cast(None, C.POINTER(C.c_double))
    x0, U = np.ascontiguousarray(prob.x0), np.ascontiguousarray(prob._U)
    tog.abi.check(gpu, gpu.tog_set_state(sm.handle.h, tog.abi.as_dp(x0), tog.abi.as_dp(U), null))
    sm.handle.solve(sm.mode)
    assert np.array_equal(sm.handle.get(tog.abi.FIELD_X), one._X) and np.array_equal(sm.handle.get(tog.abi.FIELD_U), one._U)


@pytest.mark.gpu
def test_gpu_refusals(tog, gpu):
    """8. The setter on an infeasible-start and a minimum-time handle (TOG_ERR_UNSUPPORTED with a message), on a
    problem without bound rows, for a NaN and for an infinite limit at a trimmed row (TOG_ERR_ARG; an untrimmed
    row takes it); tog_solve_pn, tog_refill, tog_refill_tables, tog_solve_stream and tog_solve_stream_tables while
    the table is set (TOG_ERR_UNSUPPORTED with a message naming the call), and again once it is cleared."""
    from test_minimum_time import pendulum_case

    lib = gpu
    ERR_ARG, ERR_UNSUPPORTED = -1, -4
    null = C.cast(None, C.POINTER(C.c_double))
    prob, opts = car_bounds(tog, 2)
    h = tog.AugmentedLagrangianSolver(prob, opts).handle
    assert h._traj_bounds
    out = np.zeros((2, tog.abi.PN_NSTATS))
    pn = tog.to_tog_pn_options(tog.ProjectedNewtonSolverOptions())
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == ERR_UNSUPPORTED
    assert b"tog_solve_pn: per-trajectory bounds" in lib.tog_last_error()
    slots = np.zeros(1, dtype=np.int32)
    sp = slots.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.tog_refill(h.h, 1, sp, tog.abi.as_dp(prob.x0[:1]), tog.abi.as_dp(prob._U[:1]), null) == ERR_UNSUPPORTED
    assert b"tog_refill: per-trajectory bounds" in lib.tog_last_error()
    xf1 = np.zeros((1, 3))
    assert lib.tog_refill_tables(h.h, 1, sp, null, null, tog.abi.as_dp(xf1)) == ERR_UNSUPPORTED
    assert b"tog_refill_tables: per-trajectory bounds" in lib.tog_last_error()
    with pytest.raises(Exception, match="tog_solve_stream: per-trajectory bounds"):
        h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U)
    with pytest.raises(Exception, match="tog_solve_stream_tables: per-trajectory bounds"):
        h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U, xf=np.tile(prob.xf, (2, 1)))
    # argument checks: the table in place stays
    T = prob.trajectory_bounds()
    bad = T.copy()
    bad[1, 3] = np.nan
    assert lib.tog_set_trajectory_bounds(h.h, tog.abi.as_dp(bad)) == ERR_ARG
    assert b"NaN at row 3 of trajectory 1" in lib.tog_last_error()
    bad = T.copy()
    bad[0, 13] = -np.inf
    assert lib.tog_set_trajectory_bounds(h.h, tog.abi.as_dp(bad)) == ERR_ARG
    assert b"infinite bound at row 13 of trajectory 0" in lib.tog_last_error()
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == ERR_UNSUPPORTED  # (still set)
    with pytest.raises(ValueError):
        h.set_trajectory_bounds(np.zeros((3, 14)))  # wrong B: refused on the host
    h.set_trajectory_bounds(None)  # cleared: projected Newton and the streamed solve run again
    h.solve(tog.abi.MODE_AL)
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == 0
    assert lib.tog_refill(h.h, 1, sp, tog.abi.as_dp(prob.x0[:1]), tog.abi.as_dp(prob._U[:1]), null) == 0
    h.set_trajectory_goals(np.tile(prob.xf, (2, 1)))  # (tog_refill_tables writes rows of a table the handle has)
    assert lib.tog_refill_tables(h.h, 1, sp, null, null, tog.abi.as_dp(np.tile(prob.xf, (1, 1)))) == 0
    h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U, xf=np.tile(prob.xf, (2, 1)))  # tog_solve_stream_tables
    h.set_trajectory_goals(None)
    h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U)  # tog_solve_stream
    # an untrimmed constraint takes an infinite limit (its descriptor may hold one), never a NaN
    pu, ou = car_bounds(tog, 2, trim=False)
    hu = tog.AugmentedLagrangianSolver(pu, ou).handle
    Tu = pu.trajectory_bounds()
    assert np.isinf(Tu).any() and hu._traj_bounds
    Tu[0, 12] = np.nan
    assert lib.tog_set_trajectory_bounds(hu.h, tog.abi.as_dp(Tu)) == ERR_ARG
    # infeasible start and minimum time
    make, aopts, xf, U0, dt, dt_mt, _ = pendulum_case(tog)
    p = make(U0, dt)
    p.X = tog.line_trajectory([0.0, 0.0], list(xf), p.N)
    for q in (tog.infeasible_problem(p, 1.0), tog.minimum_time_problem(make(U0, dt_mt, tf="min"), 15.0, 0.15, 1e-3)):
        hq = tog.AugmentedLagrangianSolver(q, aopts.opts_al).handle
        assert lib.tog_set_trajectory_bounds(hq.h, tog.abi.as_dp(np.zeros((1, 2)))) == ERR_UNSUPPORTED
        assert b"infeasible-start and minimum-time" in lib.tog_last_error()
    # no bound row
    N, n, m = 11, 3, 2
    cons = tog.Constraints(N)
    cons[N - 1] += tog.goal_constraint(np.array([0.0, 1.0, 0.0]))
    obj = tog.LQRObjective(np.eye(n), np.eye(m), np.eye(n), np.array([0.0, 1.0, 0.0]), N)
    pc = tog.Problem(tog.rk4(tog.Dynamics.car), obj, np.ones((N - 1, m)), constraints=cons, x0=np.zeros((2, n)), N=N,
                     dt=0.1)
    hc = tog.AugmentedLagrangianSolver(pc, tog.AugmentedLagrangianSolverOptions()).handle
    assert lib.tog_set_trajectory_bounds(hc.h, tog.abi.as_dp(np.zeros((2, 1)))) == ERR_ARG
    assert b"no bound row" in lib.tog_last_error()
    assert lib.tog_set_trajectory_bounds(hc.h, null) == ERR_ARG
