"""Per-trajectory cost weights within one batch (tog_set_trajectory_weights).

Trajectory b has its own Hessians Q, R, H and Qf (DevProblem::hess, a (nh, B) table of [Q; R; H; cQ; cR; Qf; cQf] that
cost_at and termh_at in csrc/tog_device.hpp read at b's block). The oracle solves one trajectory per descriptor, so
trajectory b of such a batch is held to the oracle run on ``prob.trajectory(b)``, the plain problem that carries b's
own Hessians: X, U, the statistics row and the iteration counts bit for bit, no tolerance (each figure is printed
before it is asserted).

Weight sets (seeds frozen): the car of Problems.car_obstacles at N = 21 with a goal per trajectory, bounds and two
circles, every member with its own Q, R, Qf and H, each diagonal weight scaled by 10^U(-0.5, 0.5): ``dense`` (symmetric
off-diagonals of a tenth of the smallest diagonal weight and H != 0 in every member), ``diag`` (diagonal members: the
batch keeps diag_cost >= 1) and ``mixed`` (even members diagonal, odd ones dense: trajectory 0's descriptor is
diagonal and the batch must still solve as dense); and Problems.config_quadrotor_weights(B = 6, N = 21), the
square-root path of k_expand_u and the four-wave tail kernel. ``test_inputs_are_meaningful`` holds the inputs
themselves, on the CPU, to the conditions that every member's oracle solve converges unflagged, that every member
b != 0 solves differently under trajectory 0's Hessians (what a kernel that ignored the table would compute) and that
the members' iteration counts differ.
"""
import ctypes as C
import os
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


# ----------------------------------------------------------------------------- problems


def car_weights(tog, B, kind="dense", N=21, offset=0, tables=False):
    """The car of Problems.car_obstacles (rk4, tf = 3, its bounds and two circles) at N knots with a goal and a set
    of Hessians per trajectory. Per trajectory (default_rng(9000 + offset + b), drawn in this order): U0 = 1 + 0.05
    N(0,1); the goal [0, 1, 0] + [0.05, 0.05, 0.1] U(-1, 1); the factors 10^U(-0.5, 0.5) of the 3 + 2 + 3 diagonal
    entries of Q, R, Qf = 0.01 I; the symmetric off-diagonal patterns of Q, R, Qf and the entries of H, U(-1, 1). A
    dense member adds the off-diagonals scaled to a tenth of its smallest diagonal weight (diagonally dominant, so
    positive definite) and H = 1e-3 min(weights) U(-1, 1); kind: "dense" every member, "diag" none, "mixed" the odd
    ones. tables: the bounds and the circles per trajectory too (every finite limit widened by U(0, 0.05), every
    circle moved by U(-0.02, 0.02) and its radius scaled by U(0.9, 1.1), from default_rng(9500 + offset)), so that
    the weight, goal, obstacle and bound tables are all set on one handle."""
    n, m = 3, 2
    dt = 3.0 / (N - 1)
    base = tog.Problems.car_obstacles()
    objs, U0, XF = [], [], []
    for b in range(B):
        r = np.random.default_rng(9000 + offset + b)
        U0.append(1.0 + 0.05 * r.standard_normal((N - 1, m)))
        xf = np.array([0.0, 1.0, 0.0]) + np.array([0.05, 0.05, 0.1]) * r.uniform(-1.0, 1.0, 3)
        s = 10.0 ** r.uniform(-0.5, 0.5, 2 * n + m)

        def sym(k):
            M = r.uniform(-1.0, 1.0, (k, k))
            return 0.5 * (M + M.T) * (1.0 - np.eye(k))

        oq, orr, oqf, h = sym(n), sym(m), sym(n), r.uniform(-1.0, 1.0, (m, n))
        Q, R, Qf = 0.01 * np.diag(s[0:n]), 0.01 * np.diag(s[n:n + m]), 0.01 * np.diag(s[n + m:])
        H = np.zeros((m, n))
        if kind == "dense" or (kind == "mixed" and b % 2 == 1):
            Q = Q + 0.001 * s[0:n].min() * oq
            R = R + 0.001 * s[n:n + m].min() * orr
            Qf = Qf + 0.001 * s[n + m:].min() * oqf
            H = 0.001 * min(s[0:n].min(), s[n:n + m].min()) * h
        ell = tog.QuadraticCost(Q, R, H, -Q @ xf, np.zeros(m), 0.5 * xf @ Q @ xf)
        ellN = tog.QuadraticCost(Qf, None, None, -Qf @ xf, None, 0.5 * xf @ Qf @ xf)
        objs.append(tog.Objective([ell] * (N - 1) + [ellN]))
        XF.append(xf)
    XF = np.array(XF)
    obj = tog.BatchObjective(objs, hessians="trajectory")
    bnd1, bnd = base.constraints[0][0], base.constraints[1][0]
    circ = [c for c in base.constraints[1] if isinstance(c, tog.CircleConstraints)]
    if tables:
        r = np.random.default_rng(9500 + offset)

        def widen(c):
            lim = {}
            for name, sgn in (("x_max", 1.0), ("u_max", 1.0), ("x_min", -1.0), ("u_min", -1.0)):
                v = np.tile(getattr(c, name), (B, 1))
                fin = np.isfinite(v)
                v[fin] += (sgn * r.uniform(0.0, 0.05, v.shape))[fin]
                lim[name] = v
            return tog.BoundConstraint(n, m, **lim)

        bnd1, bnd = widen(bnd1), widen(bnd)
        moved = []
        for c in circ:
            d = np.tile(c.circles, (B, 1, 1))
            d[:, :, 0:2] += r.uniform(-0.02, 0.02, d[:, :, 0:2].shape)
            d[:, :, 2] *= r.uniform(0.9, 1.1, d[:, :, 2].shape)
            moved.append(tog.CircleConstraints(n, m, d, c.label))
        circ = moved
    cons = tog.Constraints(N)
    cons[0] += bnd1
    for k in range(1, N - 1):
        cons[k] += bnd
        for c in circ:
            cons[k] += c
    cons[N - 1] += tog.goal_constraint(XF)
    prob = tog.Problem(base.model, obj, np.stack(U0), constraints=cons, x0=np.zeros((B, n)), xf=XF, N=N, dt=dt)
    return prob, tog.AugmentedLagrangianSolverOptions()


def quad_weights(tog):
    return tog.Problems.config_quadrotor_weights(B=6, N=21)


def shared_like(tog, prob):
    """the batch whose every member has trajectory 0's Hessians and its own linear terms and goal: what a handle
    without the weight table solves (the descriptor carries trajectory 0's Hessians)"""
    o0 = prob.obj[0]
    objs = []
    for o in prob.obj.objs:
        ell = tog.QuadraticCost(o0.stage.Q, o0.stage.R, o0.stage.H, o.stage.q, o.stage.r, o.stage.c)
        ellN = tog.QuadraticCost(o0.terminal.Q, None, None, o.terminal.q, None, o.terminal.c)
        objs.append(tog.Objective([ell] * (prob.N - 1) + [ellN]))
    out = prob.copy()
    out.obj = tog.BatchObjective(objs)
    assert not out.has_trajectory_weights()
    return out


BULK_B = 2304  # above the runtime's TAIL_ACTIVE = 2048: the multi-trajectory team kernels and k_al_outer in bulk


def bulk_problem(tog):
    p, opts = car_weights(tog, BULK_B, "mixed", N=11)
    opts.opts_uncon.iterations = 3
    opts.iterations = 2
    return p, opts


_ORACLE = {}


def oracle_solve(oracle, key, prob, opts):
    """Per-trajectory oracle results of prob (computed once per key, shared, never modified): {b: (X, U, steps,
    stats)} with the oracle run on prob.trajectory(b)."""
    if key not in _ORACLE:
        out = {}
        for b in range(prob.B):
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


def maxdiff(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    return float(np.nanmax(d)) if d.size else 0.0


def solve_and_compare(tog, oracle, key, prob, opts, env=None):
    """device against the oracle per member: X, U, the statistics row and the step count, bit for bit"""
    A = tog.abi
    gp = prob.copy()
    solver = with_env(env or {}, lambda: tog.solve_b(gp, opts))
    ref = oracle_solve(oracle, key, prob, opts)
    ns = A.STAT_PENALTY_MAX  # (every statistic the oracle reports: it does not fill the last entry, max μ)
    S = solver.handle.get(A.FIELD_STATS)[:, :ns]
    bad = []
    for b, (X, U, steps, st) in ref.items():
        st = st[:ns]
        dX, dU, dS = maxdiff(gp._X[b], X), maxdiff(gp._U[b], U), maxdiff(S[b], st)
        print(f"traj {b}: max|dX| {dX:.3e} max|dU| {dU:.3e} max|dstats| {dS:.3e} steps "
              f"{int(solver.stats['iterations_total'][b])} / {steps} flags {int(S[b, A.STAT_FLAGS]):#x} / "
              f"{int(st[A.STAT_FLAGS]):#x}")
        if not (np.array_equal(gp._X[b], X) and np.array_equal(gp._U[b], U) and np.array_equal(S[b], st)
                and steps == int(solver.stats["iterations_total"][b])):
            bad.append(b)
    assert not bad, bad
    return gp, solver


# ----------------------------------------------------------------------------- CPU: constructors


def test_batch_objective_hessians(tog):
    """hessians="trajectory" accepts members whose Q, R, H, Qf differ and exposes ``weights`` (B, nw), rows
    [Q; R; H; Qf] column-major; the default still raises the old text; Hessians that differ between the stage knots
    of one member raise with the trajectory and the knot named."""
    prob, _ = car_weights(tog, 4)
    obj = prob.obj
    n, m = 3, 2
    assert obj.hessians == "trajectory" and obj.weights.shape == (4, 2 * n * n + m * m + m * n)
    for b in range(4):
        st, tm = obj[b].stage, obj[b].terminal
        want = np.concatenate([st.Q.ravel(order="F"), st.R.ravel(order="F"), st.H.ravel(order="F"),
                               tm.Q.ravel(order="F")])
        assert np.array_equal(obj.weights[b], want)
        assert np.any(st.H != 0.0) and st.Q[0, 1] != 0.0 and st.Q[0, 1] == st.Q[1, 0]
    assert len({obj.weights[b].tobytes() for b in range(4)}) == 4
    # the H block is column-major: entry (i, j) of the (m, n) matrix at i + m j
    H = obj[1].stage.H
    assert obj.weights[1][n * n + m * m + 1 + m * 2] == H[1, 2]
    # as an Objective it is trajectory 0's; lin and term are built as for a shared batch
    assert obj.stage is obj[0].stage and obj.lin.shape == (4, n + m + 1) and obj.term.shape == (4, n + 1)
    assert np.array_equal(obj.lin[2], np.concatenate([obj[2].stage.q, obj[2].stage.r, [obj[2].stage.c]]))
    with pytest.raises(ValueError, match=r"trajectory 1, knot 0: Hessian Q differs from trajectory 0's"):
        tog.BatchObjective(obj.objs)
    with pytest.raises(ValueError, match="hessians must be"):
        tog.BatchObjective(obj.objs, hessians="knot")
    shared = tog.BatchObjective([obj[0], obj[0]])
    assert shared.hessians == "shared" and shared.weights is None
    same = tog.BatchObjective([obj[0], obj[0]], hessians="trajectory")
    assert np.array_equal(same.weights[0], same.weights[1])
    # one set of Hessians per trajectory: a member whose knot 3 has another R
    c = obj[2].stage
    other = tog.QuadraticCost(c.Q, 2.0 * c.R, c.H, c.q, c.r, c.c)
    costs = list(obj[2].cost)
    costs[3] = other
    with pytest.raises(ValueError, match=r"trajectory 2, knot 3: Hessian R differs from knot 0's"):
        tog.BatchObjective([obj[0], obj[1], tog.Objective(costs)], hessians="trajectory")
    # q, r, c may vary per knot as before
    costs[3] = tog.QuadraticCost(c.Q, c.R, c.H, 2.0 * c.q, c.r, c.c + 1.0)
    pk = tog.BatchObjective([obj[0], obj[1], tog.Objective(costs)], hessians="trajectory")
    assert pk.per_knot and pk.lin.shape == (3, prob.N - 1, n + m + 1) and pk.weights.shape[0] == 3


def test_lqr_objective_batch_3d(tog):
    """LQRObjectiveBatch takes (B, n, n) / (B, m, m) arrays for any of Q, R, Qf (a 2-D one is shared); member b is
    LQRObjective(Q[b], R[b], Qf[b], XF[b], N) bit for bit; a B that disagrees with XF raises."""
    rng = np.random.default_rng(3)
    n, m, N, B = 3, 2, 7, 4
    XF = rng.standard_normal((B, n))
    Q = np.stack([np.diag(rng.uniform(0.5, 2.0, n)) for _ in range(B)])
    R = np.stack([np.diag(rng.uniform(0.5, 2.0, m)) for _ in range(B)])
    Qf = np.stack([np.diag(rng.uniform(5.0, 20.0, n)) for _ in range(B)])
    for args, per in (((Q, R, Qf), True), ((Q[0], R, Qf[0]), True), ((Q[0], R[0], Qf), True),
                      ((Q[0], R[0], Qf[0]), False)):
        obj = tog.LQRObjectiveBatch(*args, XF, N)
        assert obj.hessians == ("trajectory" if per else "shared") and (obj.weights is not None) == per
        for b in range(B):
            at = [a[b] if a.ndim == 3 else a for a in args]
            one = tog.LQRObjective(at[0], at[1], at[2], XF[b], N)
            for f in ("Q", "R", "H", "q", "r"):
                assert np.array_equal(getattr(obj[b].stage, f), getattr(one.stage, f))
            assert obj[b].stage.c == one.stage.c and obj[b].terminal.c == one.terminal.c
            assert np.array_equal(obj[b].terminal.Q, one.terminal.Q) and np.array_equal(obj[b].terminal.q, one.terminal.q)
    with pytest.raises(ValueError, match="R holds the matrices of 3 trajectories, XF the goals of 4"):
        tog.LQRObjectiveBatch(Q, R[:3], Qf, XF, N)
    with pytest.raises(ValueError, match="Qf holds the matrices of 5"):
        tog.LQRObjectiveBatch(Q[0], R[0], np.concatenate([Qf, Qf[:1]]), XF, N)


def test_trajectory_round_trip_is_bitwise(tog):
    """Problem.trajectory(b) is the plain B = 1 problem carrying b's own Hessians (what the oracle is given): its
    descriptor holds them bit for bit; copy() keeps the table; batch_slice keeps a range."""
    prob, _ = car_weights(tog, 5, "mixed")
    n, m = 3, 2
    assert prob.has_trajectory_weights() and prob.has_trajectory_data() and prob.copy().has_trajectory_weights()
    W = prob.trajectory_weights()
    assert W.shape == (5, 28) and np.array_equal(prob.copy().trajectory_weights(), W) and prob.copy().obj is prob.obj
    plain = tog.Problems.car_obstacles()
    assert not plain.has_trajectory_weights() and plain.trajectory_weights() is None
    goals_only = shared_like(tog, prob)
    assert goals_only.has_trajectory_data() and goals_only.trajectory_weights() is None
    prob._X[...] = np.random.default_rng(1).standard_normal(prob._X.shape)
    for b in range(prob.B):
        t = prob.trajectory(b)
        assert t.B == 1 and not t.batched and not t.has_trajectory_data() and t.trajectory_weights() is None
        assert t.obj is prob.obj[b]
        assert np.array_equal(t.x0[0], prob.x0[b]) and np.array_equal(t._U[0], prob._U[b])
        assert np.array_equal(t._X[0], prob._X[b])
        d = t.build_desc().desc
        got = np.concatenate([np.ctypeslib.as_array(d.Q, (n * n,)), np.ctypeslib.as_array(d.R, (m * m,)),
                              np.ctypeslib.as_array(d.H, (m * n,)), np.ctypeslib.as_array(d.Qf, (n * n,))])
        assert d.batch == 1 and np.array_equal(got, W[b])
    # the batch's own descriptor carries trajectory 0's Hessians
    d = prob.build_desc().desc
    assert d.batch == 5 and np.array_equal(np.ctypeslib.as_array(d.Q, (n * n,)), W[0, 0:n * n])
    p = prob.batch_slice(1, 4)
    assert p.B == 3 and np.array_equal(p.trajectory_weights(), W[1:4]) and p.obj.hessians == "trajectory"


def test_solver_refusals_on_the_host(tog):
    """ALTRO, projected Newton and solve_stream refuse before any device call (this test runs without a device);
    Handle.set_trajectory_weights refuses a wrong shape on the host."""
    prob, opts = car_weights(tog, 3)
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.solve_b(prob.copy(), tog.ALTROSolverOptions(opts_al=opts))
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.AbstractSolverFor(prob.copy(), tog.ALTROSolverOptions(opts_al=opts))
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.solve_b(prob.copy(), tog.ProjectedNewtonSolverOptions())
    with pytest.raises(ValueError, match="per-trajectory"):
        tog.ProjectedNewtonSolver(prob.copy())
    with pytest.raises(ValueError, match="per-trajectory cost weights"):
        tog.solve_stream(prob.copy(), opts, slots=2)

    class Stub:  # (the shape check runs before the library is touched)
        n, m, B = 3, 2, 3
        set_trajectory_weights = tog.device.BatchHandle.set_trajectory_weights

    for bad in (np.zeros((2, 28)), np.zeros((3, 27)), np.zeros((3, 28, 1)), np.zeros(84)):
        with pytest.raises(ValueError, match=r"W must be \(3, 28\)"):
            Stub().set_trajectory_weights(bad)


def test_abi_mirrors(tog):
    """The entry point in the header, abi.py and libtog.jl; TOG_ABI_VERSION still 5 (a new function only)."""
    hdr = (ROOT / "include" / "tog.h").read_text()
    jl = (ROOT / "integration" / "julia" / "libtog.jl").read_text()
    assert "#define TOG_ABI_VERSION 5" in hdr and tog.abi.TOG_ABI_VERSION == 5
    assert "TOG_ABI_VERSION = Int32(5)" in jl
    name = "tog_set_trajectory_weights"
    assert f"int32_t {name}(tog_handle* h, const double* W);" in hdr
    assert f"(:{name}, libtog)" in jl and name in tog.abi.EXPORTED_SYMBOLS


def test_host_plan_under_sanitizers(tmp_path):
    """The host plan of the weight table (csrc/tog_traj_tables.hpp: the image against a direct per-member
    plan_costs, the batch's diag_cost minimum with the mixed batch, sqrt_ok, every refusal text, the part slices,
    replace_buffer under an injected allocation failure) in a stand-alone program under AddressSanitizer + UBSan
    (tests/c/traj_weights_host.cpp; no device code, no GPU)."""
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = tmp_path / "traj_weights_host"
    pkg_csrc = next(ROOT.glob("*_amd")) / "csrc"
    r = subprocess.run([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-g", "-O1", "-std=c++17", "-Wall", f"-I{pkg_csrc}",
                        str(ROOT / "tests" / "c" / "traj_weights_host.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ----------------------------------------------------------------------------- CPU: the inputs, oracle alone

FLAGGED = ("TRAJ_MAX_ITERS", "TRAJ_COST_INCREASED", "TRAJ_COST_BLOWUP", "TRAJ_MAX_REG", "TRAJ_SQRT_PD_FAIL",
           "TRAJ_AL_MAX_ITERS", "TRAJ_SINGULAR", "TRAJ_BP_ABORTED")


def _input_sets(tog):
    sets = []
    for kind in ("dense", "diag", "mixed"):
        for sqrt in (False, True):
            p, o = car_weights(tog, 5, kind)
            o.opts_uncon.square_root = sqrt
            sets.append((("car5", kind, sqrt), p, o))
    p, o = quad_weights(tog)
    sets.append((("quad6",), p, o))
    return sets


def test_inputs_are_meaningful(tog, oracle):
    """For every problem a GPU solve test below uses: each member's oracle solve ends AL_CONVERGED with none of the
    limit or exception flags; each member b != 0 ends on another X than under trajectory 0's Hessians (its own
    linear terms and goal kept: what a kernel that ignored the table would solve); at least two members differ in
    their iteration count. The quadrotor's longest member outlasts the second longest by several steps, so the
    compacted tail launches of a narrowing batch run."""
    A = tog.abi
    bad = sum(getattr(A, n) for n in FLAGGED)
    for key, p, o in _input_sets(tog):
        ref = oracle_solve(oracle, key, p, o)
        ign = oracle_solve(oracle, key + ("ignored",), shared_like(tog, p), o)
        steps = []
        for b, (X, U, st_n, st) in ref.items():
            f = int(st[A.STAT_FLAGS])
            print(key, b, st_n, hex(f), "under trajectory 0's Hessians:", ign[b][2])
            assert f & A.TRAJ_AL_CONVERGED and not f & bad, (key, b, hex(f))
            assert np.isfinite(X).all() and np.isfinite(U).all(), (key, b)
            if b == 0:
                assert np.array_equal(X, ign[0][0]) and st_n == ign[0][2], key
            else:
                assert not np.array_equal(X, ign[b][0]), (key, b)
            steps.append(st_n)
        assert len(set(steps)) >= 2, (key, steps)
        if key[0] == "quad6":
            top = sorted(steps)
            assert top[-1] - top[-2] >= 5, steps


def test_config_quadrotor_weights(tog):
    """Problems.config_quadrotor_weights: config 3's starts and options, a positive diagonal scaling of Q, R and Qf
    within the documented range, every member its own; N keeps the final time."""
    P = tog.Problems
    prob, opts = P.config_quadrotor_weights(B=8)
    base, bopts = P.config_quadrotor(B=8)
    n, m = 13, 4
    assert prob.N == 101 and prob.dt == base.dt and opts.opts_uncon.square_root
    assert np.array_equal(prob.x0, base.x0) and np.array_equal(prob._U, base._U) and np.array_equal(prob.xf, base.xf)
    W = prob.trajectory_weights()
    assert W.shape == (8, 2 * n * n + m * m + m * n) and len({W[b].tobytes() for b in range(8)}) == 8
    lo, hi = 10.0 ** -P.QUAD_WEIGHTS_LOG10, 10.0 ** P.QUAD_WEIGHTS_LOG10
    for b in range(8):
        st, tm = prob.obj[b].stage, prob.obj[b].terminal
        for M, M0 in ((st.Q, base.obj.stage.Q), (st.R, base.obj.stage.R), (tm.Q, base.obj.terminal.Q)):
            s = np.diag(M) / np.diag(M0)
            assert np.all((s >= lo * (1 - 1e-12)) & (s <= hi * (1 + 1e-12))) and len(set(s.tolist())) == len(s)
            off = M[~np.eye(len(M), dtype=bool)]
            assert np.all(off == 0.0) and not np.signbit(off).any()
        assert np.all(st.H == 0.0)
    short, _ = P.config_quadrotor_weights(B=6, N=21)
    assert short.N == 21 and short.B == 6 and short.dt * 20 == pytest.approx(base.dt * 100)
    assert np.array_equal(short.trajectory_weights(), W[:6]) and np.array_equal(short._U, base._U[:6, :20])
    assert short.constraints.num_constraints()[-1] == base.constraints.num_constraints()[-1]


# ----------------------------------------------------------------------------- GPU

ENVS = {"default": {}, "team": {"TOG_BWD_TAIL": "team"}, "full": {"TOG_NO_COMPACT": "1"}, "lds": {"TOG_BWD": "lds"}}


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
@pytest.mark.parametrize("kernels", list(ENVS))
def test_gpu_car_dense(tog, oracle, gpu, sqrt, kernels):
    """4. Car, B = 5 (four teams to a wave: a team wave holds different trajectories), each member its own
    non-diagonal Q, Qf, R and H != 0, with a goal per trajectory, bounds and circles; AL, std and square root; the
    default kernels, the one-wave team tail kernel, uncompacted launches and the LDS backward kernel."""
    prob, opts = car_weights(tog, 5, "dense")
    opts.opts_uncon.square_root = sqrt
    gp, solver = solve_and_compare(tog, oracle, ("car5", "dense", sqrt), prob, opts, ENVS[kernels])
    assert solver.handle._traj_weights
    assert np.all(tog.max_violation(gp) < opts.constraint_tolerance)


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
@pytest.mark.parametrize("kind", ["diag", "mixed"])
def test_gpu_car_diagonal_and_mixed(tog, oracle, gpu, kind, sqrt):
    """5. All-diagonal members (the batch keeps diag_cost >= 1: the diagonal forms of the run-time-structure
    kernels), and the mixed batch: trajectory 0, whose Hessians the descriptor carries, is diagonal, trajectory 1 is
    dense, and the batch must solve as dense."""
    prob, opts = car_weights(tog, 5, kind)
    opts.opts_uncon.square_root = sqrt
    st0, st1 = prob.obj[0].stage, prob.obj[1].stage
    assert np.all(st0.H == 0.0) and st0.Q[0, 1] == 0.0 and (np.any(st1.H != 0.0)) == (kind == "mixed")
    solve_and_compare(tog, oracle, ("car5", kind, sqrt), prob, opts)


@pytest.mark.gpu
def test_gpu_quadrotor_weights(tog, oracle, gpu):
    """6. config_quadrotor_weights(B = 6, N = 21), AL + square root: the stage knots' expansion on k_expand_u's 4-lane
    teams and the four-wave k_bwd_quad tail. One member outlasts the others by several steps (asserted from the
    statistics), so the batch narrows and the compacted tail launches run down to a single trajectory."""
    prob, opts = quad_weights(tog)
    assert opts.opts_uncon.square_root
    gp, solver = solve_and_compare(tog, oracle, ("quad6",), prob, opts)
    steps = np.sort(solver.stats["iterations_total"])
    assert steps[-1] - steps[-2] >= 5 and len(set(steps.tolist())) >= 3, steps
    assert np.all(solver.stats["c_max"] < opts.constraint_tolerance)


def test_step_inputs(tog):
    """(CPU) the step-level problem carries all four tables"""
    prob, _ = car_weights(tog, 5, "dense", tables=True)
    assert prob.has_trajectory_weights() and prob.has_trajectory_bounds() and prob.has_trajectory_obstacles()
    assert prob.trajectory_goals() is not None and prob.trajectory_obstacles().shape == (5, 2, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
def test_gpu_step_level(tog, oracle, gpu, sqrt):
    """7. One tog_solve_step with the weight, goal, obstacle and bound tables all on one handle: K, d, ΔV and the
    line search's result (J, α, z, the trial count, the accepted X and U) against the oracle's step on
    prob.trajectory(b), bit for bit. The oracle's step is ilqr_iterate's: Jacobians, expansion, backward pass,
    forward pass from the initial rollout's cost."""
    A = tog.abi
    prob, opts = car_weights(tog, 5, "dense", tables=True)
    opts.opts_uncon.square_root = sqrt
    h = tog.AugmentedLagrangianSolver(prob, opts).handle
    assert h._traj_weights and h._traj_bounds and h._traj_obstacles and h._traj_goals and h._traj_costs
    h.solve_init(A.MODE_AL)
    h.solve_step(1)
    K, d, dV = h.get(A.FIELD_K), h.get(A.FIELD_D), h.get(A.FIELD_DV)
    X, U, S = h.get(A.FIELD_X), h.get(A.FIELD_U), h.get(A.FIELD_STATS)
    bad = []
    for b in range(prob.B):
        o = oracle.OracleSolver(prob.trajectory(b), opts, b=0)
        o.rollout_open_loop()
        J0 = o.cost(True)
        o.jacobians()
        assert o.cost_expansion(sqrt, True) == 0
        dVo, _ = o.backward(sqrt)
        J = o.forward(J0, True)
        st = o.get("stats")
        got = (S[b, A.STAT_J], S[b, A.STAT_ALPHA], S[b, A.STAT_Z], S[b, A.STAT_LS_TRIALS])
        want = (J, st[A.STAT_ALPHA], st[A.STAT_Z], st[A.STAT_LS_TRIALS])
        print(f"traj {b}: max|dK| {maxdiff(K[b], o.get('K')):.3e} max|dd| {maxdiff(d[b], o.get('d')):.3e} dV "
              f"{dV[b].tolist()} / {dVo.tolist()} (J, alpha, z, trials) {got} / {want} max|dX| "
              f"{maxdiff(X[b], o.get('Xbar')):.3e} max|dU| {maxdiff(U[b], o.get('Ubar')):.3e}")
        ok = (np.array_equal(K[b], o.get("K")) and np.array_equal(d[b], o.get("d")) and np.array_equal(dV[b], dVo)
              and got == want and want[1] > 0.0
              and np.array_equal(X[b], o.get("Xbar")) and np.array_equal(U[b], o.get("Ubar")))
        if not ok:
            bad.append(b)
    assert not bad, bad
    assert len({K[b].tobytes() for b in range(prob.B)}) == prob.B


def _handle_solve(tog, h, mode):
    h.solve(mode)
    return h.get(tog.abi.FIELD_X), h.get(tog.abi.FIELD_U), h.get(tog.abi.FIELD_STATS)


@pytest.mark.gpu
@pytest.mark.parametrize("sqrt", [False, True])
def test_gpu_set_clear_and_upload_state(tog, gpu, sqrt):
    """8. Handle life cycle on the mixed batch, whose table changes the handle's diag_cost from the descriptor's
    (trajectory 0 is diagonal) to dense: set the table (upload_state with a weights problem), solve, clear it
    (upload_state with a plain one, then NULL directly), solve: bitwise a fresh shared handle's result, on a
    square-root handle too; then the table again: bitwise the first result."""
    prob, opts = car_weights(tog, 5, "mixed")
    opts.opts_uncon.square_root = sqrt
    shared = shared_like(tog, prob)
    fresh_w, fresh_s = prob.copy(), shared.copy()
    sw, ss = tog.solve_b(fresh_w, opts), tog.solve_b(fresh_s, opts)
    Sw, Ss = sw.handle.get(tog.abi.FIELD_STATS), ss.handle.get(tog.abi.FIELD_STATS)
    assert not np.array_equal(fresh_w._X[1:], fresh_s._X[1:])
    assert not ss.handle.__dict__.get("_traj_weights", False)
    solver = tog.AugmentedLagrangianSolver(prob, opts)
    h = solver.handle
    assert h._traj_weights
    X, U, S = _handle_solve(tog, h, solver.mode)
    assert np.array_equal(X, fresh_w._X) and np.array_equal(U, fresh_w._U) and np.array_equal(S, Sw)
    h.upload_state(shared)  # (a problem without the table clears it: NULL)
    assert not h._traj_weights and h._traj_costs
    X, U, S = _handle_solve(tog, h, solver.mode)
    assert np.array_equal(X, fresh_s._X) and np.array_equal(U, fresh_s._U) and np.array_equal(S, Ss)
    h.upload_state(prob)
    assert h._traj_weights
    X, U, S = _handle_solve(tog, h, solver.mode)
    assert np.array_equal(X, fresh_w._X) and np.array_equal(U, fresh_w._U) and np.array_equal(S, Sw)
    h.upload_state(prob)
    h.set_trajectory_weights(None)  # the setter itself
    X, U, S = _handle_solve(tog, h, solver.mode)
    assert np.array_equal(X, fresh_s._X) and np.array_equal(U, fresh_s._U) and np.array_equal(S, Ss)


@pytest.mark.gpu
def test_gpu_multi_handle_slices(tog, gpu):
    """8. tog_create_multi over devices [0, 0], B = 5: the slices of 3 and 2 receive their own blocks. A table with
    a NaN in the second part's slice is refused whole: both parts keep their tables."""
    prob, opts = car_weights(tog, 5, "dense")
    one = prob.copy()
    s1 = tog.solve_b(one, opts)
    two = prob.copy()
    sm = tog.AugmentedLagrangianSolver(two, opts, devices=[0, 0])
    tog.solve_b(two, sm)
    assert np.array_equal(one._X, two._X) and np.array_equal(one._U, two._U)
    assert np.array_equal(s1.handle.get(tog.abi.FIELD_STATS), sm.handle.get(tog.abi.FIELD_STATS))
    bad = np.ascontiguousarray(prob.trajectory_weights() * 1.5)  # (other weights everywhere: a part that took its
    bad[4, 9] = np.nan                                           # slice would solve differently)
    assert gpu.tog_set_trajectory_weights(sm.handle.h, tog.abi.as_dp(bad)) == -1
    assert b"trajectory 4: R has a NaN" in gpu.tog_last_error()
    null = C.cast(None, C.POINTER(C.c_double))
    x0, U = np.ascontiguousarray(prob.x0), np.ascontiguousarray(prob._U)
    tog.abi.check(gpu, gpu.tog_set_state(sm.handle.h, tog.abi.as_dp(x0), tog.abi.as_dp(U), null))
    sm.handle.solve(sm.mode)
    assert np.array_equal(sm.handle.get(tog.abi.FIELD_X), one._X) and np.array_equal(sm.handle.get(tog.abi.FIELD_U), one._U)


@pytest.mark.gpu
def test_gpu_refusals(tog, gpu):
    """9. TOG_ERR_ARG with the trajectory and the matrix named: a NaN, an infinity, a Q, R or Qf that is not
    symmetric, and on a square-root handle a Hessian that is not positive definite (a handle without square_root
    takes it); the table in place stays. TOG_ERR_UNSUPPORTED: the setter on an infeasible-start and a minimum-time
    handle and on a handle with a time-varying stage_costs table; tog_solve_pn, tog_refill, tog_refill_tables,
    tog_solve_stream and tog_solve_stream_tables while the table is set, with a message naming the call. The same
    calls succeed once the table is cleared. (No handle carries a GenericCost: it is not a solver cost.)"""
    from test_minimum_time import pendulum_case

    lib = gpu
    ERR_ARG, ERR_UNSUPPORTED = -1, -4
    null = C.cast(None, C.POINTER(C.c_double))
    prob, opts = car_weights(tog, 2, "dense")
    h = tog.AugmentedLagrangianSolver(prob, opts).handle
    assert h._traj_weights
    out = np.zeros((2, tog.abi.PN_NSTATS))
    pn = tog.to_tog_pn_options(tog.ProjectedNewtonSolverOptions())
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == ERR_UNSUPPORTED
    assert b"tog_solve_pn: per-trajectory" in lib.tog_last_error()
    h.set_trajectory_costs(None, None)  # (the cost and goal tables have refusals of their own: the weights' alone)
    h.set_trajectory_goals(None)
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == ERR_UNSUPPORTED
    assert b"tog_solve_pn: per-trajectory cost weights" in lib.tog_last_error()
    slots = np.zeros(1, dtype=np.int32)
    sp = slots.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.tog_refill(h.h, 1, sp, tog.abi.as_dp(prob.x0[:1]), tog.abi.as_dp(prob._U[:1]), null) == ERR_UNSUPPORTED
    assert b"tog_refill: per-trajectory cost weights" in lib.tog_last_error()
    xf1 = np.zeros((1, 3))
    assert lib.tog_refill_tables(h.h, 1, sp, null, null, tog.abi.as_dp(xf1)) == ERR_UNSUPPORTED
    assert b"tog_refill_tables: per-trajectory cost weights" in lib.tog_last_error()
    with pytest.raises(Exception, match="tog_solve_stream: per-trajectory cost weights"):
        h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U)
    with pytest.raises(Exception, match="tog_solve_stream_tables: per-trajectory cost weights"):
        h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U, xf=np.tile(prob.xf[0], (2, 1)))
    # argument checks: the table in place stays
    W = prob.trajectory_weights()
    n, m = 3, 2
    oR, oH, oQf = n * n, n * n + m * m, n * n + m * m + m * n
    for (b, i, v), msg in (((1, oH + 2, np.nan), b"trajectory 1: H has a NaN or an infinite entry"),
                           ((0, oQf + 4, np.inf), b"trajectory 0: Qf has a NaN or an infinite entry"),
                           ((1, 0, -np.inf), b"trajectory 1: Q has a NaN or an infinite entry"),
                           ((1, 1, 0.5), b"trajectory 1: Q is not symmetric"),
                           ((0, oR + 2, 0.5), b"trajectory 0: R is not symmetric"),
                           ((1, oQf + 3, 0.5), b"trajectory 1: Qf is not symmetric")):
        bad = W.copy()
        bad[b, i] = v
        assert lib.tog_set_trajectory_weights(h.h, tog.abi.as_dp(bad)) == ERR_ARG, msg
        assert msg in lib.tog_last_error(), lib.tog_last_error()
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == ERR_UNSUPPORTED  # (still set)
    with pytest.raises(ValueError):
        h.set_trajectory_weights(np.zeros((3, 28)))  # wrong B: refused on the host
    # positive definiteness: asked of a square-root handle only, as tog_create asks it of the shared Hessians
    notpd = W.copy()
    notpd[1, oR + 3] = 0.0  # R(1, 1) of trajectory 1: R = [[r, o], [o, 0]] is indefinite
    assert lib.tog_set_trajectory_weights(h.h, tog.abi.as_dp(notpd)) == 0
    assert lib.tog_set_trajectory_weights(h.h, tog.abi.as_dp(W)) == 0
    so = tog.AugmentedLagrangianSolverOptions()
    so.opts_uncon.square_root = True
    hs = tog.AugmentedLagrangianSolver(prob, so).handle
    assert lib.tog_set_trajectory_weights(hs.h, tog.abi.as_dp(notpd)) == ERR_ARG
    assert b"trajectory 1: R is not positive definite" in lib.tog_last_error()
    notpd = W.copy()
    notpd[0, oQf] = -1.0
    assert lib.tog_set_trajectory_weights(hs.h, tog.abi.as_dp(notpd)) == ERR_ARG
    assert b"trajectory 0: Qf is not positive definite" in lib.tog_last_error()
    # cleared: projected Newton and the streamed solves run again
    h.set_trajectory_weights(None)
    h.solve(tog.abi.MODE_AL)
    assert lib.tog_solve_pn(h.h, C.byref(pn), tog.abi.as_dp(out)) == 0
    assert lib.tog_refill(h.h, 1, sp, tog.abi.as_dp(prob.x0[:1]), tog.abi.as_dp(prob._U[:1]), null) == 0
    h.set_trajectory_goals(np.tile(prob.xf[0], (2, 1)))  # (tog_refill_tables writes rows of a table the handle has)
    assert lib.tog_refill_tables(h.h, 1, sp, null, null, tog.abi.as_dp(np.tile(prob.xf[0], (1, 1)))) == 0
    h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U, xf=np.tile(prob.xf[0], (2, 1)))  # tog_solve_stream_tables
    h.set_trajectory_goals(None)
    h.solve_stream(tog.abi.MODE_AL, prob.x0, prob._U)  # tog_solve_stream
    # infeasible start and minimum time
    make, aopts, xf, U0, dt, dt_mt, _ = pendulum_case(tog)
    p = make(U0, dt)
    p.X = tog.line_trajectory([0.0, 0.0], list(xf), p.N)
    for q in (tog.infeasible_problem(p, 1.0), tog.minimum_time_problem(make(U0, dt_mt, tf="min"), 15.0, 0.15, 1e-3)):
        hq = tog.AugmentedLagrangianSolver(q, aopts.opts_al).handle
        nw = 2 * hq.n * hq.n + hq.m * hq.m + hq.m * hq.n
        assert lib.tog_set_trajectory_weights(hq.h, tog.abi.as_dp(np.zeros((1, nw)))) == ERR_UNSUPPORTED
        assert b"tog_set_trajectory_weights: infeasible-start and minimum-time" in lib.tog_last_error()
    # a time-varying objective: the handle came with a stage_costs table
    N = prob.N
    st, tm = prob.obj[0].stage, prob.obj[0].terminal
    costs = [tog.QuadraticCost((1.0 + 0.1 * k) * st.Q, st.R, st.H, st.q, st.r, st.c) for k in range(N - 1)]
    tv = tog.Problem(prob.model, tog.Objective(costs + [tm]), prob._U.copy(), constraints=prob.trajectory(0).constraints,
                     x0=prob.x0.copy(), xf=prob.xf[0], N=N, dt=prob.dt)
    ht = tog.AugmentedLagrangianSolver(tv, opts).handle
    assert lib.tog_set_trajectory_weights(ht.h, tog.abi.as_dp(W)) == ERR_UNSUPPORTED
    assert b"time-varying stage_costs table" in lib.tog_last_error()


@pytest.mark.gpu
def test_gpu_width_independence(tog, gpu):
    """10. The car at N = 11, mixed members, B = 2304 (above the runtime's TAIL_ACTIVE = 2048: the multi-trajectory
    team kernels in bulk) with 3 inner and 2 outer iterations: bitwise equal to the same trajectories solved as two
    batches of 1152."""
    prob, opts = bulk_problem(tog)
    gp = prob.copy()
    solver = tog.solve_b(gp, opts)
    S = solver.handle.get(tog.abi.FIELD_STATS)
    assert solver.handle._traj_weights
    half = BULK_B // 2
    for lo in (0, half):
        p = prob.batch_slice(lo, lo + half)
        s = tog.solve_b(p, opts)
        assert np.array_equal(p._X, gp._X[lo:lo + half]) and np.array_equal(p._U, gp._U[lo:lo + half]), lo
        assert np.array_equal(s.handle.get(tog.abi.FIELD_STATS), S[lo:lo + half]), lo
    assert len({gp._X[b].tobytes() for b in (0, 1, half, BULK_B - 1)}) == 4
