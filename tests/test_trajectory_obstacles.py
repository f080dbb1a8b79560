"""Per-trajectory obstacles within one batch (tog_set_trajectory_obstacles).

The batch shares the kind and number of its circle and sphere rows; trajectory b has its own centres and radii
(DevProblem::obs, a (4, no, B) table read by traj_row in csrc/tog_device.hpp at the row's obstacle ordinal). The
oracle solves one trajectory per descriptor, so trajectory b of such a batch is held to the oracle run on
``prob.trajectory(b)``, the plain problem of b: X, U within 1e-6 relative, equal iteration counts and STAT_J within
1e-6 relative (TOL_SOLVE and the step contract of tests/test_trajectory_goals.py); step-level quantities bit for
bit, because the arithmetic is the shared problem's and only where a row's a, b, c, r come from differs.

Obstacle sets (seeds frozen): set A, the car among two circles held by two separate CircleConstraints objects,
centres moved by U(-0.05, 0.05) and radii scaled by U(0.9, 1.1); set B, the quadrotor past three spheres, centres
moved by U(-1, 1) per coordinate and radii scaled by U(0.9, 1.1). The CPU test
``test_inputs_converge_in_the_oracle`` holds the inputs themselves to the condition that every trajectory's oracle
solve ends AL_CONVERGED within the options' limits with no exception flag.
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


def swap_constraints(tog, prob, swap):
    """prob with the constraint objects in swap (id -> replacement) replaced at every knot"""
    cons = tog.Constraints(prob.N)
    for k in range(prob.N):
        cons[k] = tog.ConstraintSet(swap.get(id(c), c) for c in prob.constraints[k])
    out = tog.Problem(prob.model, prob.obj, constraints=cons, x0=prob.x0, xf=prob.xf, N=prob.N, dt=prob.dt)
    out._U[...] = prob._U
    return out


def car_circles(tog, B, offset=0, jitter=True):
    """Set A: Problems.car_obstacles with U0 = 1 + 0.05 N(0,1), and both circles (two CircleConstraints objects)
    moved by U(-0.05, 0.05) per coordinate with the radius scaled by U(0.9, 1.1). One default_rng(7000 + offset +
    b) per trajectory, drawn in the order U0, then per constraint the centre, then the radius. jitter = False keeps
    the problem's own circles in every trajectory (the table equals the descriptor's data)."""
    N, m = 51, 2
    U0, d = [], []
    for b in range(B):
        r = np.random.default_rng(7000 + offset + b)
        U0.append(1.0 + 0.05 * r.standard_normal((N - 1, m)))
        d.append([np.concatenate([r.uniform(-0.05, 0.05, 2), r.uniform(0.9, 1.1, 1)]) for _ in range(2)])
    d = np.array(d)  # (B, 2 constraints, [dx, dy, scale])
    prob = tog.Problems.car_obstacles(U0=np.stack(U0))
    obs = [c for c in prob.constraints[1] if isinstance(c, tog.CircleConstraints)]
    assert len(obs) == 2
    swap = {}
    for j, c in enumerate(obs):
        circ = np.tile(c.circles, (B, 1, 1))
        if jitter:
            circ[:, 0, 0:2] += d[:, j, 0:2]
            circ[:, 0, 2] *= d[:, j, 2]
        swap[id(c)] = tog.CircleConstraints(3, 2, circ, c.label)
    return swap_constraints(tog, prob, swap), tog.AugmentedLagrangianSolverOptions()


QUAD_MEMBERS = (1, 2, 3, 4, 5)  # of config_quadrotor(B = 8); members 0 and 6 end AL_MAX_ITERS in the oracle


def quad_spheres(tog):
    """Set B: quadrotor_test("goal+bounds+obs") with x0, U0 of config_quadrotor(B = 8)'s members 1..5, the three
    spheres moved by U(-1, 1) per coordinate and their radii scaled by U(0.9, 1.1) (default_rng(7200 + s): the
    centre offsets (3, 3), then the radius factors (3,)). Config 3's options (square root)."""
    base, opts = tog.Problems.config_quadrotor(B=8)
    s = list(QUAD_MEMBERS)
    prob = tog.Problems.quadrotor_test("goal+bounds+obs", x0=base.x0[s].copy(), U0=base._U[s].copy())
    sph0 = next(c for c in prob.constraints[0] if isinstance(c, tog.SphereConstraints))
    sph = np.tile(sph0.spheres, (len(s), 1, 1))
    for i, member in enumerate(s):
        r = np.random.default_rng(7200 + member)
        sph[i, :, 0:3] += r.uniform(-1.0, 1.0, (3, 3))
        sph[i, :, 3] *= r.uniform(0.9, 1.1, 3)
    return swap_constraints(tog, prob, {id(sph0): tog.SphereConstraints(13, 4, sph, sph0.label)}), opts


BULK_B = 2304  # above the runtime's TAIL_ACTIVE = 2048: the multi-trajectory team kernels and k_al_outer in bulk
BULK_CHECK = (0, 63, 64, 1151, 1152, 2047, 2048, BULK_B - 1)  # first, a wave boundary, the halves' seam, 2048, last


def bulk_problem(tog):
    p, opts = car_circles(tog, BULK_B)
    opts.opts_uncon.iterations = 3
    opts.iterations = 2
    return p, opts


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


def test_shapes_and_for_traj(tog):
    """(no, w) is the shared constraint, (B, no, w) holds a set per trajectory: batched, for_traj(b) is the plain
    constraint of b, to_abi carries trajectory 0's data, length counts the obstacles."""
    rng = np.random.default_rng(0)
    c1 = tog.CircleConstraints(3, 2, [[0.1, 0.2, 0.3], [1.0, 2.0, 3.0]])
    assert not c1.batched and c1.for_traj(4) is c1 and c1.length() == 2 and c1.length("terminal") == 0
    cb = tog.CircleConstraints(3, 2, rng.standard_normal((4, 2, 3)), "cyl")
    assert cb.batched and cb.length() == 2 and cb.label == "cyl"
    sb = tog.SphereConstraints(13, 4, rng.standard_normal((4, 3, 4)))
    assert sb.batched and sb.length() == 3
    assert not tog.SphereConstraints(13, 4, [(0.0, 1.0, 2.0, 3.0)]).batched
    for con, data, w in ((cb, cb.circles, 3), (sb, sb.spheres, 4)):
        for b in range(4):
            t = con.for_traj(b)
            assert type(t) is type(con) and not t.batched and t.label == con.label
            assert np.array_equal(t.circles if w == 3 else t.spheres, data[b])
        kind, count, flat = con.to_abi()
        assert count == data.shape[1] and np.array_equal(flat, data[0].ravel())
        assert kind == (tog.abi.CON_CIRCLES if w == 3 else tog.abi.CON_SPHERES)
    x, u = np.array([0.3, -0.2, 0.1]), np.zeros(2)
    assert np.array_equal(cb.evaluate(x, u), cb.for_traj(0).evaluate(x, u))
    with pytest.raises(ValueError, match=r"\(B, no, 3\)"):
        tog.CircleConstraints(3, 2, np.zeros((4, 2, 4)))
    with pytest.raises(ValueError, match=r"\(B, no, 4\)"):
        tog.SphereConstraints(13, 4, np.zeros((4, 2, 3)))


def test_trajectory_round_trip_is_bitwise(tog):
    """Problem.trajectory(b) is the plain B = 1 problem of b: its circles and spheres, x0, U, X, bit for bit, one
    plain object per batched one (knots that share a set keep sharing it); copy() keeps the data."""
    prob, _ = tog.Problems.config_quad_maze_obstacles(B=5, N=11)
    assert prob.has_trajectory_data() and prob.has_trajectory_obstacles() and prob.copy().has_trajectory_data()
    T = prob.trajectory_obstacles()
    assert T.shape == (5, 7, 4) and np.array_equal(prob.copy().trajectory_obstacles(), T)
    plain, _ = tog.Problems.config_quad_maze(B=5, N=11)
    assert not plain.has_trajectory_data() and plain.trajectory_obstacles() is None
    assert np.array_equal(plain.x0, prob.x0) and np.array_equal(plain._U, prob._U)
    prob._X[...] = np.random.default_rng(1).standard_normal(prob._X.shape)
    cyl = next(c for c in prob.constraints[1] if isinstance(c, tog.CircleConstraints))
    sph = next(c for c in prob.constraints[1] if isinstance(c, tog.SphereConstraints))
    for b in range(prob.B):
        t = prob.trajectory(b)
        assert t.B == 1 and not t.batched and not t.has_trajectory_data() and t.trajectory_obstacles() is None
        assert np.array_equal(t.x0[0], prob.x0[b]) and np.array_equal(t._U[0], prob._U[b])
        assert np.array_equal(t._X[0], prob._X[b])
        tc = [c for c in t.constraints[1] if isinstance(c, tog.CircleConstraints)]
        ts = [c for c in t.constraints[1] if isinstance(c, tog.SphereConstraints)]
        assert len(tc) == 1 and len(ts) == 1
        assert np.array_equal(tc[0].circles, cyl.circles[b]) and np.array_equal(ts[0].spheres, sph.spheres[b])
        assert t.constraints[2][1] is tc[0] and t.constraints[2][2] is ts[0]  # (shared across knots)
        # the table's row of b is the plain problem's descriptor data: [x, y, 0, r] and [x, y, z, r]
        assert np.array_equal(T[b][:4][:, [0, 1, 3]], cyl.circles[b]) and np.all(T[b, :4, 2] == 0.0)
        assert np.array_equal(T[b, 4:], sph.spheres[b])
        d = t.build_desc()
        assert d.desc.batch == 1
    # the perturbation is the documented one: centres within 1 m, radii within 10 %
    c0 = next(c for c in plain.constraints[1] if isinstance(c, tog.CircleConstraints)).circles
    assert np.all(np.abs(cyl.circles[:, :, :2] - c0[:, :2]) <= 1.0)
    assert np.all(np.abs(cyl.circles[:, :, 2] / c0[:, 2] - 1.0) <= 0.1 + 1e-12)
    assert len({cyl.circles[b].tobytes() for b in range(5)}) == 5


def test_batch_slice(tog):
    prob, _ = car_circles(tog, 6)
    T = prob.trajectory_obstacles()
    p = prob.batch_slice(2, 5)
    assert p.B == 3 and p.has_trajectory_obstacles()
    assert np.array_equal(p.trajectory_obstacles(), T[2:5])
    assert np.array_equal(p.x0, prob.x0[2:5]) and np.array_equal(p._U, prob._U[2:5])
    for b in range(3):
        a, c = p.trajectory(b), prob.trajectory(2 + b)
        for ca, cc in zip(a.constraints[1], c.constraints[1]):
            if isinstance(ca, tog.CircleConstraints):
                assert np.array_equal(ca.circles, cc.circles)


def test_trajectory_obstacles_order(tog):
    """The ordinal order of the ABI: sets in the descriptor's order (first appearance over the knots; the terminal
    knot's set is its own), constraints in their set's order, then the constraint's own order. Two objects in one
    set follow each other; one object in two distinct sets is emitted once per set."""
    n, m, N, B = 3, 2, 6, 3
    rng = np.random.default_rng(3)
    Q = np.eye(n)
    obj = tog.LQRObjective(Q, np.eye(m), Q, np.zeros(n), N)
    model = tog.rk4(tog.Dynamics.car)
    a = tog.CircleConstraints(n, m, rng.standard_normal((B, 2, 3)), "a")
    b = tog.CircleConstraints(n, m, rng.standard_normal((1, 3)), "b")  # shared data beside batched data
    bnd = tog.BoundConstraint(n, m, u_min=-1.0, u_max=1.0)

    def rows(c):
        return c.obstacle_rows(B)

    # two objects in one set
    cons = tog.Constraints(N)
    for k in range(1, N - 1):
        cons[k] += bnd
        cons[k] += a
        cons[k] += b
    p = tog.Problem(model, obj, constraints=cons, x0=np.zeros((B, n)), N=N, dt=0.1)
    T = p.trajectory_obstacles()
    assert T.shape == (B, 3, 4)
    assert np.array_equal(T[:, :2], rows(a)) and np.array_equal(T[:, 2:], rows(b))
    assert np.array_equal(T[1, 0], [a.circles[1, 0, 0], a.circles[1, 0, 1], 0.0, a.circles[1, 0, 2]])
    assert np.array_equal(T[2, 2], [b.circles[0, 0], b.circles[0, 1], 0.0, b.circles[0, 2]])
    # one object in two distinct sets: knots 1-2 hold [bnd, a], knots 3-4 hold [b, a]
    cons = tog.Constraints(N)
    for k in (1, 2):
        cons[k] += bnd
        cons[k] += a
    for k in (3, 4):
        cons[k] += b
        cons[k] += a
    p = tog.Problem(model, obj, constraints=cons, x0=np.zeros((B, n)), N=N, dt=0.1)
    T = p.trajectory_obstacles()
    assert T.shape == (B, 5, 4)
    assert np.array_equal(T[:, 0:2], rows(a)) and np.array_equal(T[:, 2:3], rows(b))
    assert np.array_equal(T[:, 3:5], rows(a))
    d = p.build_desc().desc
    assert d.n_sets == 2 and [d.knot_set[k] for k in range(N)] == [-1, 0, 0, 1, 1, -1]


def test_wrong_batch_raises(tog):
    prob, _ = car_circles(tog, 3)
    with pytest.raises(ValueError, match="obstacles of 3 trajectories, the problem 2 trajectories"):
        tog.Problem(prob.model, prob.obj, constraints=prob.constraints, x0=prob.x0[:2], N=prob.N, dt=prob.dt)
    quad, _ = quad_spheres(tog)
    with pytest.raises(ValueError, match="SphereConstraints holds the obstacles of 5 trajectories, the problem 4"):
        tog.Problem(quad.model, quad.obj, constraints=quad.constraints, x0=quad.x0[:4], N=quad.N, dt=quad.dt)


def test_max_violation_honours_each_obstacle_set(tog):
    """Every trajectory against its own obstacles: trajectory 1 sits inside its own first circle, which lies
    outside trajectory 0's and 2's circles."""
    prob, _ = car_circles(tog, 3)
    obs1 = next(c for c in prob.constraints[1] if isinstance(c, tog.CircleConstraints))
    circ = obs1.circles.copy()
    circ[1, 0] = [0.0, 0.3, 0.1]  # trajectory 1's first circle, away from everyone else's
    prob = swap_constraints(tog, prob, {id(obs1): tog.CircleConstraints(3, 2, circ, obs1.label)})
    prob._X[...] = 0.0
    prob._X[:, :, 1] = 0.3  # every state at (0, 0.3): the centre of that circle
    prob._U[...] = 1.0  # inside the control bounds
    prob._X[:, -1] = prob.xf  # the goal
    v = tog.max_violation(prob)
    assert v[0] == 0.0 and v[2] == 0.0
    assert v[1] == 0.1 ** 2


def test_solver_refusals_on_the_host(tog):
    """ALTRO, projected Newton and solve_stream refuse before any device call (this test runs without a device)."""
    prob, opts = car_circles(tog, 3)
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.solve_b(prob.copy(), tog.ALTROSolverOptions(opts_al=opts))
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.AbstractSolverFor(prob.copy(), tog.ALTROSolverOptions(opts_al=opts))
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.solve_b(prob.copy(), tog.ProjectedNewtonSolverOptions())
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.ProjectedNewtonSolver(prob.copy())
    with pytest.raises(ValueError, match="per-trajectory obstacles"):
        tog.solve_stream(prob.copy(), opts, slots=2)


def test_abi_mirrors(tog):
    """The entry point in the header, abi.py and libtog.jl; TOG_ABI_VERSION still 5 (a new function only)."""
    hdr = (ROOT / "include" / "tog.h").read_text()
    jl = (ROOT / "integration" / "julia" / "libtog.jl").read_text()
    assert "#define TOG_ABI_VERSION 5" in hdr and tog.abi.TOG_ABI_VERSION == 5
    assert "TOG_ABI_VERSION = Int32(5)" in jl
    name = "tog_set_trajectory_obstacles"
    assert f"int32_t {name}(tog_handle* h, const double* obs);" in hdr
    assert f"(:{name}, libtog)" in jl and name in tog.abi.EXPORTED_SYMBOLS


def test_host_plan_under_sanitizers(tmp_path):
    """The host plan of the obstacle table (csrc/tog_traj_tables.hpp: ordinals, no, the table image, the part
    slices, the error texts) in a stand-alone program under AddressSanitizer + UBSan
    (tests/c/traj_obstacles_host.cpp; no device code, no GPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "traj_obstacles_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "traj_obstacles_host.cpp"), "-o", str(exe)],
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
        p, o = car_circles(tog, 5)
        o.opts_uncon.square_root = sqrt
        sets.append((("car5", sqrt), p, o, None, True))
    p, o = quad_spheres(tog)
    sets.append((("quad5",), p, o, None, True))
    p, o = bulk_problem(tog)
    sets.append((("bulk",), p, o, BULK_CHECK, False))  # (iterations capped: held to "no exception" only)
    return sets


def test_inputs_converge_in_the_oracle(tog, oracle):
    """For every obstacle set a GPU test below uses, each trajectory's oracle solve ends AL_CONVERGED within the
    options' iteration limits with no exception flag and finite X, U. The bulk set runs under capped iteration
    counts (its test compares bits, not convergence), so its eight oracle-checked trajectories are held to the
    absence of exception flags."""
    for key, p, o, trajs, must_converge in _input_sets(tog):
        ref = oracle_solve(oracle, key, p, o, trajs)
        for b, (X, U, steps, st) in ref.items():
            f, exc = _flags(tog, st)
            print(key, b, steps, hex(f))
            assert exc == 0, (key, b, f)
            assert np.isfinite(X).all() and np.isfinite(U).all(), (key, b)
            if must_converge:
                assert f & tog.abi.TRAJ_AL_CONVERGED, (key, b, f)
                assert not f & tog.abi.TRAJ_AL_MAX_ITERS, (key, b, f)


# ----------------------------------------------------------------------------- GPU

ENVS = {"default": {}, "team": {"TOG_BWD_TAIL": "team"}, "full": {"TOG_NO_COMPACT": "1"}, "lds": {"TOG_BWD": "lds"}}


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
@pytest.mark.parametrize("kernels", list(ENVS))
def test_gpu_car_circles(tog, oracle, gpu, sqrt, kernels):
    """5. Set A, B = 5 (with four teams to a wave, five trajectories fill one wave of teams and leave a partial
    one): two circles in two constraint objects, each trajectory its own, on the default kernels, the one-wave
    team tail kernel, uncompacted launches and the LDS backward kernel."""
    prob, opts = car_circles(tog, 5)
    opts.opts_uncon.square_root = sqrt
    solve_and_compare(tog, oracle, ("car5", sqrt), prob, opts, ENVS[kernels])


@pytest.mark.gpu
def test_gpu_quadrotor_spheres(tog, oracle, gpu):
    """6. Set B: quadrotor AL, bounds + three spheres + goal, square root; c_max and the host max_violation below
    the tolerance for every trajectory against its own spheres."""
    prob, opts = quad_spheres(tog)
    gp, solver = solve_and_compare(tog, oracle, ("quad5",), prob, opts)
    assert np.all(solver.stats["c_max"] < opts.constraint_tolerance)
    assert np.all(tog.max_violation(gp) < opts.constraint_tolerance)  # (host side, each against its own spheres)


def _maze_step_problem(tog):
    """config_quad_maze_obstacles(B = 5, N = 11) with seeded X, U: knot k of trajectory b sits near the centre of
    its own obstacle (k - 1) mod 7 (inside it: the row is active), the other states and the controls random."""
    prob, opts = tog.Problems.config_quad_maze_obstacles(B=5, N=11)
    T = prob.trajectory_obstacles()
    rng = np.random.default_rng(11)
    prob._X[...] = rng.standard_normal(prob._X.shape)
    prob._U[...] = tog.Problems.HOVER + rng.standard_normal(prob._U.shape)
    for b in range(prob.B):
        for k in range(1, prob.N - 1):
            o = T[b, (k - 1) % 7]
            prob._X[b, k, 0:2] = o[0:2] + 0.3 * o[3] * rng.uniform(-1.0, 1.0, 2)
            prob._X[b, k, 2] = (o[2] if (k - 1) % 7 >= 4 else 10.0) + 0.3 * o[3] * rng.uniform(-1.0, 1.0)
    return prob, opts


def test_step_inputs_have_active_obstacle_rows(tog, oracle):
    """The step-level inputs, on the oracle alone: every trajectory has an obstacle row with c > 0, at every
    knot that holds obstacle rows."""
    prob, opts = _maze_step_problem(tog)
    for b in range(prob.B):
        t = prob.trajectory(b)
        o = oracle.OracleSolver(t, opts, b=0)
        o.update_constraints()
        Co = o.get("C")
        nb = sum(c.length() for c in t.constraints[1] if isinstance(c, tog.BoundConstraint))
        for k in range(1, prob.N - 1):
            assert np.max(Co[k, nb:nb + 7]) > 0.0, (b, k)


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
def test_gpu_step_level(tog, oracle, gpu, sqrt):
    """7. Step level, B = 5, cylinders, spheres and state bounds in one set: tog_cost (al 0 and 1), TOG_FIELD_C
    after tog_update_constraints and TOG_FIELD_Q after tog_cost_expansion (std or square root), each trajectory
    against the oracle on its own problem, bit for bit."""
    prob, opts = _maze_step_problem(tog)
    h = tog.AugmentedLagrangianSolver(prob, opts).handle
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
        nb = sum(c.length() for c in t.constraints[1] if isinstance(c, tog.BoundConstraint))
        assert np.max(Co[1:prob.N - 1, nb:nb + 7]) > 0.0, b  # an active obstacle row
        assert J0[b] == j0 and J1[b] == j1, b
        assert np.array_equal(Cd[b], Co), b
        assert o.cost_expansion(sqrt, True) == 0
        assert np.array_equal(Qd[b], o.get("Q")), b
    # the same kind of X, U costs differently per trajectory (the table is read per trajectory)
    assert len(set(J1.tolist())) == prob.B


@pytest.mark.gpu
def test_gpu_bulk_kernels(tog, oracle, gpu):
    """8. Set A's generator at B = 2304 with 3 inner and 2 outer iterations: above TAIL_ACTIVE = 2048, so the
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


@pytest.mark.gpu
def test_gpu_equal_tables_equal_shared_problem(tog, gpu):
    """9. A table of B copies of the descriptor's data: X, U and FIELD_STATS are bitwise the plain problem's."""
    same, opts = car_circles(tog, 4, jitter=False)
    assert same.has_trajectory_obstacles()
    plain = tog.Problems.car_obstacles(U0=same._U.copy())
    assert not plain.has_trajectory_data()
    a, b = plain.copy(), same.copy()
    sa, sb = tog.solve_b(a, opts), tog.solve_b(b, opts)
    assert np.array_equal(a._X, b._X) and np.array_equal(a._U, b._U)
    assert np.array_equal(sa.handle.get(tog.abi.FIELD_STATS), sb.handle.get(tog.abi.FIELD_STATS))


def _handle_solve(tog, h, mode):
    h.solve(mode)
    return h.get(tog.abi.FIELD_X), h.get(tog.abi.FIELD_U), h.get(tog.abi.FIELD_STATS)


@pytest.mark.gpu
def test_gpu_retargeting(tog, gpu):
    """10. Solve, set another table on the same handle, solve again: bitwise a fresh handle's result. NULL returns
    to the shared result (the descriptor's circles, trajectory 0's, for every trajectory)."""
    first, opts = car_circles(tog, 4)
    second, _ = car_circles(tog, 4, offset=50)
    second._U[...] = first._U  # same starts: only the obstacles change
    assert not np.array_equal(first.trajectory_obstacles(), second.trajectory_obstacles())
    fresh = second.copy()
    sf = tog.solve_b(fresh, opts)
    Sf = sf.handle.get(tog.abi.FIELD_STATS)
    solver = tog.AugmentedLagrangianSolver(first, opts)
    h = solver.handle
    X1, _, _ = _handle_solve(tog, h, solver.mode)
    h.upload_state(first)  # x0, U, X = NaN again
    h.set_trajectory_obstacles(second.trajectory_obstacles())
    X, U, S = _handle_solve(tog, h, solver.mode)
    assert np.array_equal(X, fresh._X) and np.array_equal(U, fresh._U) and np.array_equal(S, Sf)
    assert not np.array_equal(X, X1)
    # back to the descriptor's obstacles: trajectory 0 of `first` for everyone
    T0 = first.trajectory_obstacles()[0]
    shared = tog.Problems.car_obstacles(U0=first._U.copy())
    obs = [c for c in shared.constraints[1] if isinstance(c, tog.CircleConstraints)]
    shared = swap_constraints(tog, shared, {id(c): tog.CircleConstraints(3, 2, T0[j:j + 1, [0, 1, 3]], c.label)
                                            for j, c in enumerate(obs)})
    assert not shared.has_trajectory_data()
    ref = shared.copy()
    ss = tog.solve_b(ref, opts)
    h.upload_state(shared)  # (a problem without per-trajectory data clears the table: NULL)
    assert not h._traj_obstacles
    X, U, S = _handle_solve(tog, h, solver.mode)
    assert np.array_equal(X, ref._X) and np.array_equal(U, ref._U)
    assert np.array_equal(S, ss.handle.get(tog.abi.FIELD_STATS))


@pytest.mark.gpu
def test_gpu_multi_handle_slices(tog, gpu):
    """11. tog_create_multi over devices [0, 0], B = 5: the slices of 3 and 2 receive their own rows."""
    prob, opts = car_circles(tog, 5)
    one = prob.copy()
    s1 = tog.solve_b(one, opts)
    two = prob.copy()
    sm = tog.AugmentedLagrangianSolver(two, opts, devices=[0, 0])
    tog.solve_b(two, sm)
    assert np.array_equal(one._X, two._X) and np.array_equal(one._U, two._U)
    assert np.array_equal(s1.handle.get(tog.abi.FIELD_STATS), sm.handle.get(tog.abi.FIELD_STATS))


@pytest.mark.gpu
def test_gpu_refusals(tog, gpu):
    """12. The setter on an infeasible-start and a minimum-time handle (TOG_ERR_UNSUPPORTED with a message) and on
    a problem without obstacle rows (TOG_ERR_ARG); tog_solve_pn, tog_refill and tog_solve_stream while the table
    is set (TOG_ERR_UNSUPPORTED), and again once it is cleared."""
    from test_minimum_time import pendulum_case

    lib = gpu
    ERR_ARG, ERR_UNSUPPORTED = -1, -4
    null = C.cast(None, C.POINTER(C.c_double))
    prob, opts = car_circles(tog, 2)
    h = tog.AugmentedLagrangianSolver(prob, opts).handle
    out = np.zeros((2, tog.abi.PN_NSTATS))
    pn = tog.to_tog_pn_options(tog.ProjectedNewtonSolverOptions())
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == ERR_UNSUPPORTED
    assert b"per-trajectory obstacles" in lib.tog_last_error()
    slots = np.zeros(1, dtype=np.int32)
    sp = slots.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.tog_refill(h.h, 1, sp, tog.abi.as_dp(prob.x0[:1]), tog.abi.as_dp(prob._U[:1]), null) == ERR_UNSUPPORTED
    assert b"tog_refill: per-trajectory obstacles" in lib.tog_last_error()
    with pytest.raises(Exception, match="per-trajectory obstacles"):
        h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U)
    h.set_trajectory_obstacles(None)  # cleared: projected Newton runs again
    h.solve(tog.abi.MODE_AL)
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == 0
    with pytest.raises(ValueError):
        h.set_trajectory_obstacles(np.zeros((3, 2, 4)))  # wrong B: refused on the host
    # infeasible start and minimum time
    make, aopts, xf, U0, dt, dt_mt, _ = pendulum_case(tog)
    p = make(U0, dt)
    p.X = tog.line_trajectory([0.0, 0.0], list(xf), p.N)
    for q in (tog.infeasible_problem(p, 1.0), tog.minimum_time_problem(make(U0, dt_mt, tf="min"), 15.0, 0.15, 1e-3)):
        hq = tog.AugmentedLagrangianSolver(q, aopts.opts_al).handle
        assert lib.tog_set_trajectory_obstacles(hq.h, tog.abi.as_dp(np.zeros((1, 1, 4)))) == ERR_UNSUPPORTED
        assert b"infeasible-start and minimum-time" in lib.tog_last_error()
    # no circle or sphere constraint
    pc, oc = tog.Problems.config_quadrotor(B=2)
    hc = tog.AugmentedLagrangianSolver(pc, oc).handle
    assert lib.tog_set_trajectory_obstacles(hc.h, tog.abi.as_dp(np.zeros((2, 1, 4)))) == ERR_ARG
    assert b"no circle or sphere" in lib.tog_last_error()
    assert lib.tog_set_trajectory_obstacles(hc.h, null) == ERR_ARG
