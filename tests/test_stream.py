"""Streamed solves: J jobs through the B trajectory slots of one handle (tog_finished, tog_get_slots, tog_refill,
tog_refill_tables, tog_solve_stream, tog_solve_stream_tables; Python ``solve_stream``).

A slot whose trajectory finished is harvested and given the next queued job while the other slots keep iterating.
A trajectory's result does not depend on the slot, the step or the launch widths that served it, so every streamed
job must equal the same job solved in one plain batch bit for bit; against the CPU oracle the bound is the solve
level one of the other tests (1e-6 relative on X and U, equal iteration counts).

Job sets (seeds frozen): config 2's cartpole starts (``config_cartpole``, seeds 1000 + job) and the car among two
circles (``car_obstacles``) with U0 = 1 + 0.3 N(0, 1) (seed 5000 + job); the goal sweep is
tests/test_trajectory_goals.py's ``cartpole_goals``. ``test_inputs_spread_in_the_oracle`` holds these sets to two
conditions under the oracle alone: every job converges within the options' limits with no exception flag, and the
jobs' step counts differ by at least a factor of two, so that slots free up at different times and refills
interleave with running trajectories. (The bulk set's 12,305 jobs are held to them at the jobs the test picks.)
"""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from test_trajectory_goals import cartpole_goals, rel

ROOT = pathlib.Path(__file__).resolve().parent.parent
TOL_SOLVE = 1e-6

STREAM_FUNCTIONS = ("tog_finished", "tog_get_slots", "tog_refill", "tog_refill_tables", "tog_solve_stream",
                    "tog_solve_stream_tables")

SMALL_J, SMALL_B = 29, 8   # cartpole, iLQR: B <= TAIL_ACTIVE, every step after the first readback is compacted
CAR_J, CAR_B = 13, 4       # car among circles, AL
BULK_B = 4096              # above TAIL_ACTIVE = 2048, and B x 21 trials > 65536: line searches pend across steps
BULK_J = 3 * BULK_B + 17
# first, wave seams, the slot count's seam (the last job of the first fill, the first refilled), later seams, last
BULK_CHECK = (0, 63, 64, BULK_B - 1, BULK_B, 2 * BULK_B - 1, 2 * BULK_B, 3 * BULK_B, BULK_J - 1)
GOAL_J, GOAL_B = 21, 8


# ----------------------------------------------------------------------------- job sets


def cartpole_jobs(tog, J, offset=0):
    return tog.Problems.config_cartpole(B=J, offset=offset)


def car_jobs(tog, J, seed0=5000):
    N, m = 51, 2
    U0 = np.stack([1.0 + 0.3 * np.random.default_rng(seed0 + b).standard_normal((N - 1, m)) for b in range(J)])
    return tog.Problems.car_obstacles(U0=U0), tog.AugmentedLagrangianSolverOptions()


def bulk_pick(tog):
    """The bulk set's picked jobs as a small problem of their own (job BULK_CHECK[i] is its trajectory i)."""
    N, m = 101, 1
    U0 = np.stack([0.01 + 0.5 * np.random.default_rng(1000 + j).standard_normal((N - 1, m)) for j in BULK_CHECK])
    prob, opts = tog.Problems.config_cartpole(B=len(BULK_CHECK))
    prob._U[...] = U0
    return prob, opts


_ORACLE = {}


def oracle_jobs(oracle, tog, key, prob, opts, jobs):
    """{job: (X, U, steps, flags)} from the oracle on prob.trajectory(job); computed once per (key, job), shared,
    never modified."""
    out = {}
    for j in jobs:
        if (key, j) not in _ORACLE:
            o = oracle.OracleSolver(prob.trajectory(j), opts, b=0)
            steps = o.solve()
            X, U = o.get("X"), o.get("U")
            X.setflags(write=False)
            U.setflags(write=False)
            _ORACLE[(key, j)] = (X, U, steps, int(o.get("stats")[tog.abi.STAT_FLAGS]))
        out[j] = _ORACLE[(key, j)]
    return out


def mode_of(tog, opts):
    return tog.abi.MODE_AL if isinstance(opts, tog.AugmentedLagrangianSolverOptions) else tog.abi.MODE_ILQR


# ----------------------------------------------------------------------------- CPU


def test_abi_mirrors_present(tog):
    """The new entry points are declared in the header, mirrored in abi.py and libtog.jl, and exported by the
    library; they are new functions only, so the ABI version stays 5 and says so."""
    header = (ROOT / "include" / "tog.h").read_text()
    jl = (ROOT / "integration" / "julia" / "libtog.jl").read_text()
    lib = tog.abi.load_library()
    for f in STREAM_FUNCTIONS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % f, header), f
        assert f in tog.abi.EXPORTED_SYMBOLS, f
        assert hasattr(lib, f), f
        assert "(:%s, libtog)" % f in jl, f
    assert tog.abi.TOG_ABI_VERSION == 5 and lib.tog_version() == 5
    assert re.search(r"still 5.*new functions only", header, re.S)
    assert callable(tog.solve_stream)


def test_stream_without_device_fails_loudly(tog):
    """No CPU path: a null handle is TOG_ERR_ARG with a message, and without a HIP device ``solve_stream``
    raises from the handle's creation (TOG_ERR_DEVICE) instead of computing anywhere else."""
    lib = tog.abi.load_library()
    null = C.cast(None, C.POINTER(C.c_double))
    done = C.c_int64(-1)
    rc = lib.tog_solve_stream(None, 0, 1, null, null, null, null, null, 0, C.byref(done))
    assert rc == tog.abi.ERR_ARG and lib.tog_last_error()
    cnt = C.c_int32()
    assert lib.tog_finished(None, None, C.byref(cnt)) == tog.abi.ERR_ARG
    assert lib.tog_refill(None, 0, None, null, null, null) == tog.abi.ERR_ARG
    if lib.tog_device_count() > 0:
        return  # (a device is visible: the GPU tests below run the real thing)
    prob, opts = cartpole_jobs(tog, 5)
    with pytest.raises(RuntimeError, match="libtog error -2"):
        tog.solve_stream(prob, opts, slots=2)


def test_solve_stream_argument_checks(tog):
    prob, opts = cartpole_jobs(tog, 3)
    with pytest.raises(ValueError):
        tog.solve_stream(prob, tog.ALTROSolverOptions())
    with pytest.raises(ValueError):
        tog.solve_stream(prob, tog.ProjectedNewtonSolverOptions())
    given = prob.copy()
    given._X[...] = 0.0
    with pytest.raises(ValueError):
        tog.solve_stream(given, opts)
    # batch_slice: the slice's members, bit for bit
    gp, _ = cartpole_goals(tog, 5)
    s = gp.batch_slice(1, 4)
    assert s.B == 3 and np.array_equal(s.x0, gp.x0[1:4]) and np.array_equal(s._U, gp._U[1:4])
    assert np.array_equal(s.obj.lin, gp.obj.lin[1:4]) and np.array_equal(s.obj.term, gp.obj.term[1:4])
    assert np.array_equal(s.xf, gp.xf[1:4])


def test_inputs_spread_in_the_oracle(tog, oracle):
    """Every job of the sets below converges in the oracle within the options' limits with no exception flag, and
    the step counts within a set differ by at least a factor of two between the fastest and the slowest job."""
    A = tog.abi
    bad = (A.TRAJ_MAX_ITERS | A.TRAJ_COST_INCREASED | A.TRAJ_COST_BLOWUP | A.TRAJ_MAX_REG | A.TRAJ_SQRT_PD_FAIL |
           A.TRAJ_AL_MAX_ITERS | A.TRAJ_SINGULAR | A.TRAJ_BP_ABORTED)
    sets = []
    p, o = cartpole_jobs(tog, SMALL_J)
    sets.append(("small", p, o, A.TRAJ_CONVERGED))
    p, o = car_jobs(tog, CAR_J)
    sets.append(("car", p, o, A.TRAJ_AL_CONVERGED))
    p, o = cartpole_goals(tog, GOAL_J)
    sets.append(("goals", p, o, A.TRAJ_CONVERGED))
    p, o = bulk_pick(tog)
    sets.append(("bulk", p, o, A.TRAJ_CONVERGED))
    for key, prob, opts, good in sets:
        ref = oracle_jobs(oracle, tog, key, prob, opts, range(prob.B))
        steps = [ref[j][2] for j in range(prob.B)]
        print(key, steps)
        for j in range(prob.B):
            assert ref[j][3] & good and not ref[j][3] & bad, (key, j, ref[j][3])
        assert max(steps) >= 2 * min(steps), (key, steps)


# ----------------------------------------------------------------------------- GPU


def _handle(tog, prob, opts, history=0):
    solver = tog.AbstractSolverFor(prob, opts, device=0)
    if history:
        solver.handle.enable_history(history)
    return solver


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cartpole_ilqr", "car_al"])
def test_refill_equals_init(tog, gpu, case):
    """tog_refill leaves a slot as tog_set_state + tog_solve_init leave it, bit for bit: handle A is initialised
    with the inputs; handle B runs other inputs to the end and is then refilled, all 8 slots in a scrambled
    order, with A's inputs."""
    A = tog.abi
    if case == "cartpole_ilqr":
        prob, opts = cartpole_jobs(tog, 8)
        other, _ = cartpole_jobs(tog, 8, offset=100)
    else:
        prob, opts = car_jobs(tog, 8)
        other, _ = car_jobs(tog, 8, seed0=5100)
    mode = mode_of(tog, opts)
    cap = 16
    a = _handle(tog, prob.copy(), opts, cap).handle
    a.solve_init(mode)
    b = _handle(tog, other.copy(), opts, cap).handle
    b.solve(mode)
    assert not np.any(b.status() & A.TRAJ_ACTIVE)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4], dtype=np.int32)  # job i -> slot perm[i]
    b.refill(perm, prob.x0, prob._U)
    fields = [A.FIELD_X, A.FIELD_U, A.FIELD_X0, A.FIELD_D, A.FIELD_RHO, A.FIELD_STATS]
    if mode == A.MODE_AL:
        fields += [A.FIELD_C, A.FIELD_LAMBDA, A.FIELD_MU]
    for f in fields:
        fa, fb = a.get(f), b.get(f)
        assert np.array_equal(fa, fb[perm], equal_nan=True), f
    sa, sb = a.get(A.FIELD_STATS), b.get(A.FIELD_STATS)
    assert np.all(sa[:, A.STAT_FLAGS] == A.TRAJ_ACTIVE) and np.all(sb[:, A.STAT_ITERATIONS] == 1)
    assert np.all(np.isfinite(sa[:, A.STAT_J]))
    ia, oa, ca = a.history()
    ib, ob, cb = b.history()
    assert np.array_equal(ca, cb[perm]) and np.all(ca[:, 0] == 1)
    assert np.array_equal(ia[:, 0], ib[perm][:, 0])
    if mode == A.MODE_AL:
        assert np.all(ca[:, 1] == 1) and np.array_equal(oa[:, 0], ob[perm][:, 0])
    # tog_get_slots serves the same blocks, in list order
    for f in (A.FIELD_X, A.FIELD_STATS, A.FIELD_HIST_INNER, A.FIELD_HIST_COUNT):
        got = b.get_slots(f, perm)
        want = {A.FIELD_HIST_INNER: ib, A.FIELD_HIST_COUNT: cb.astype(float)}.get(f)
        want = b.get(f) if want is None else want
        assert np.array_equal(got, want[perm], equal_nan=True), f


def _plain(tog, prob, opts):
    p = prob.copy()
    s = tog.solve_b(p, opts, history=False)
    return p, s.handle.get(tog.abi.FIELD_STATS)


def _check_stream(tog, oracle, key, prob, opts, slots, jobs_oracle):
    A = tog.abi
    plain, Sp = _plain(tog, prob, opts)
    sp = prob.copy()
    solver = tog.solve_stream(sp, opts, slots=slots)
    Ss = np.stack([solver.stats[k] for k in ("iterations", "iterations_total", "flags")])
    assert solver.stats["jobs_done"] == prob.B
    assert np.array_equal(plain._X, sp._X) and np.array_equal(plain._U, sp._U)
    assert np.array_equal(Ss[0], Sp[:, A.STAT_ITERATIONS].astype(np.int64))
    assert np.array_equal(Ss[1], Sp[:, A.STAT_TOTAL_STEPS].astype(np.int64))
    assert np.array_equal(Ss[2], Sp[:, A.STAT_FLAGS].astype(np.int64))
    assert np.array_equal(solver.stats["cost"], Sp[:, A.STAT_J])
    assert not np.any(Ss[2] & A.TRAJ_ACTIVE)
    ref = oracle_jobs(oracle, tog, key, prob, opts, jobs_oracle)
    for j, (X, U, steps, flags) in ref.items():
        eX, eU = rel(sp._X[j], X), rel(sp._U[j], U)
        print(f"{key} job {j}: errX {eX:.3e} errU {eU:.3e} steps {int(Ss[1][j])} / {steps}")
        assert eX < TOL_SOLVE and eU < TOL_SOLVE, j
        assert steps == int(Ss[1][j]), j
    return sp, solver


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cartpole_ilqr", "car_al"])
def test_small_stream_compacted_tail(tog, gpu, oracle, case):
    """B <= TAIL_ACTIVE: every step after the first readback is a compacted launch over k_list_active's list, so
    a refilled slot that the list or the launch width missed would never be stepped (and its job never end).
    Every job equals the same job in one plain batch of J bit for bit; jobs 0, B-1, B (the first refilled) and J-1
    equal the oracle."""
    if case == "cartpole_ilqr":
        (prob, opts), B, key = cartpole_jobs(tog, SMALL_J), SMALL_B, "small"
    else:
        (prob, opts), B, key = car_jobs(tog, CAR_J), CAR_B, "car"
    _check_stream(tog, oracle, key, prob, opts, B, (0, B - 1, B, prob.B - 1))


@pytest.mark.gpu
def test_bulk_stream_pending_line_searches(tog, gpu, oracle):
    """4,096 slots, J = 3 x 4096 + 17: above TAIL_ACTIVE, and line searches pend across steps (B x 21 > 65536), so
    a job is refilled into a slot whose previous occupant may have left ls_pend or candidate state behind. Bit
    for bit the plain batches of the same jobs (X, U, iteration counts, flags: the fields
    tests/test_line_search_modes.py compares across schedules), at every job; the picked jobs also equal the
    oracle."""
    A = tog.abi
    prob, opts = cartpole_jobs(tog, BULK_J)
    sp = prob.copy()
    solver = tog.solve_stream(sp, opts, slots=BULK_B)
    assert solver.stats["jobs_done"] == BULK_J
    for lo in range(0, BULK_J, BULK_B):
        hi = min(lo + BULK_B, BULK_J)
        plain, S = _plain(tog, prob.batch_slice(lo, hi), opts)
        assert np.array_equal(plain._X, sp._X[lo:hi]), lo
        assert np.array_equal(plain._U, sp._U[lo:hi]), lo
        assert np.array_equal(S[:, A.STAT_TOTAL_STEPS].astype(np.int64), solver.stats["iterations_total"][lo:hi]), lo
        assert np.array_equal(S[:, A.STAT_FLAGS].astype(np.int64), solver.stats["flags"][lo:hi]), lo
    pick, _ = bulk_pick(tog)
    for i, j in enumerate(BULK_CHECK):
        assert np.array_equal(pick._U[i], prob._U[j])  # (the picked problem is the bulk set's jobs)
    ref = oracle_jobs(oracle, tog, "bulk", pick, opts, range(len(BULK_CHECK)))
    for i, j in enumerate(BULK_CHECK):
        X, U, steps, _ = ref[i]
        assert rel(sp._X[j], X) < TOL_SOLVE and rel(sp._U[j], U) < TOL_SOLVE, j
        assert steps == int(solver.stats["iterations_total"][j]), j


@pytest.mark.gpu
def test_step_level_loop_equals_driver(tog, gpu):
    """The J = 29 stream written over tog_solve_step / tog_finished / tog_get_slots / tog_refill equals
    tog_solve_stream's output bit for bit; tog_refill refuses an active slot and a slot listed twice."""
    A = tog.abi
    prob, opts = cartpole_jobs(tog, SMALL_J)
    J, B = SMALL_J, SMALL_B
    sp = prob.copy()
    drv = tog.solve_stream(sp, opts, slots=B)
    h = _handle(tog, prob.batch_slice(0, B), opts).handle
    lib = h.lib
    h.solve_init(A.MODE_ILQR)
    # every slot is active now
    one = np.array([0], dtype=np.int32)
    two = np.array([1, 1], dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    x0, U0 = np.ascontiguousarray(prob.x0), np.ascontiguousarray(prob._U)
    rc = lib.tog_refill(h.h, 1, one.ctypes.data_as(ip), A.as_dp(x0), A.as_dp(U0), None)
    assert rc == A.ERR_ARG and b"active" in lib.tog_last_error()
    rc = lib.tog_refill(h.h, 2, two.ctypes.data_as(ip), A.as_dp(x0), A.as_dp(U0), None)
    assert rc == A.ERR_ARG and b"twice" in lib.tog_last_error()
    job_of = list(range(B))
    nxt, out = B, 0
    X = np.zeros_like(prob._X)
    U = np.zeros_like(prob._U)
    S = np.zeros((J, A.NSTATS))
    for _ in range(10000):
        h.solve_step(4)
        fin = h.finished()
        if len(fin) == 0:
            continue
        jobs = [job_of[s] for s in fin]
        assert all(j >= 0 for j in jobs)
        X[jobs] = h.get_slots(A.FIELD_X, fin)
        U[jobs] = h.get_slots(A.FIELD_U, fin)
        S[jobs] = h.get_slots(A.FIELD_STATS, fin)
        out += len(fin)
        for s in fin:
            job_of[s] = -1
        take = fin[:min(len(fin), J - nxt)]
        if len(take):
            new = list(range(nxt, nxt + len(take)))
            h.refill(take, x0[new], U0[new])
            for s, j in zip(take, new):
                job_of[s] = j
            nxt += len(take)
        if out == J:
            break
    assert out == J
    assert np.array_equal(X, sp._X) and np.array_equal(U, sp._U)
    assert np.array_equal(S[:, A.STAT_TOTAL_STEPS].astype(np.int64), drv.stats["iterations_total"])
    assert np.array_equal(S[:, A.STAT_FLAGS].astype(np.int64), drv.stats["flags"])
    assert np.array_equal(S[:, A.STAT_J], drv.stats["cost"])
    assert len(h.finished()) == 0  # every finished slot was listed once


@pytest.mark.gpu
def test_goal_sweep_stream(tog, gpu, oracle):
    """21 goals through 8 slots (solve_stream routes a BatchObjective through tog_solve_stream_tables): every job
    matches the oracle on its single-goal problem and equals one solve_b batch of the 21 bit for bit."""
    prob, opts = cartpole_goals(tog, GOAL_J)
    _check_stream(tog, oracle, "goals", prob, opts, GOAL_B, range(GOAL_J))


@pytest.mark.gpu
def test_budget_and_refusals(tog, gpu):
    A = tog.abi
    prob, opts = cartpole_jobs(tog, SMALL_J)
    sp = prob.copy()
    solver = tog.solve_stream(sp, opts, slots=SMALL_B, max_steps=8)  # TOG_OK: no exception
    st = solver.stats
    done = st["jobs_done"]
    assert done < SMALL_J
    S = np.stack([st["iterations"], st["iterations_total"], st["flags"]], axis=1)
    never = np.all(S == 0, axis=1) & (st["cost"] == 0.0)
    started = ~never
    assert never.any() and started.sum() >= SMALL_B
    assert not never[:SMALL_B].any() and np.all(np.diff(never.astype(int)) >= 0)  # the queue is served in order
    active = (st["flags"] & A.TRAJ_ACTIVE) != 0
    assert int((started & ~active).sum()) == done
    assert np.all(st["iterations_total"][started & active] <= 8)
    assert np.all(np.isfinite(sp._X[started]))
    # refusals
    lib = solver.handle.lib
    null = C.cast(None, C.POINTER(C.c_double))
    x0, U0 = np.ascontiguousarray(prob.x0), np.ascontiguousarray(prob._U)
    cnt = C.c_int64()
    rc = lib.tog_solve_stream_tables(solver.handle.h, A.MODE_ILQR, SMALL_J, A.as_dp(x0), A.as_dp(U0), null, null,
                                     null, null, null, null, 0, C.byref(cnt))
    assert rc == A.ERR_UNSUPPORTED and lib.tog_last_error()
    multi = tog.AbstractSolverFor(prob.batch_slice(0, SMALL_B), opts, devices=[0, 0]).handle
    rc = lib.tog_solve_stream(multi.h, A.MODE_ILQR, SMALL_J, A.as_dp(x0), A.as_dp(U0), null, null, null, 0,
                              C.byref(cnt))
    assert rc == A.ERR_UNSUPPORTED and b"tog_create_multi" in lib.tog_last_error()
    slots = np.zeros(1, dtype=np.int32)
    c32 = C.c_int32()
    assert lib.tog_finished(multi.h, slots.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(c32)) == A.ERR_UNSUPPORTED
