"""``BatchHandle``: one ``tog_handle`` (include/tog.h) = one problem x B trajectories resident in
HBM on one GPU. Thin ctypes plumbing; all compute happens in libtog.so (HIP, gfx950).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi


class BatchHandle:
    def __init__(self, prob, opts: abi.tog_options, device: int = 0, stream=None, devices=None):
        """``devices``: a list of HIP device ids for one handle over several GPUs
        (tog_create_multi: the batch is split into contiguous slices, one per entry)."""
        self.lib = abi.load_library()
        self.hcap = 0
        self.desc_builder = prob.build_desc()
        self.opts = opts
        h = C.c_void_p()
        if devices is not None:
            devs = np.ascontiguousarray(np.asarray(devices, dtype=np.int32))
            abi.check(self.lib, self.lib.tog_create_multi(C.byref(self.desc_builder.desc), C.byref(opts),
                                                          devs.ctypes.data_as(C.POINTER(C.c_int32)), len(devs),
                                                          C.byref(h)))
        else:
            abi.check(self.lib, self.lib.tog_create(C.byref(self.desc_builder.desc), C.byref(opts), int(device),
                                                    C.byref(h)))
        self.h = h
        dims = (C.c_int64 * 6)()
        abi.check(self.lib, self.lib.tog_dims(self.h, dims))
        self.n, self.m, self.N, self.B, self.pmax, _ = [int(v) for v in dims]
        if stream is not None:
            abi.check(self.lib, self.lib.tog_set_stream(self.h, C.c_void_p(int(stream))))
        self.upload_state(prob)

    @classmethod
    def adopt(cls, lib, handle: int, opts: abi.tog_options):
        """Wrap a ``tog_handle`` created inside libtog (tog_solve_altro_ex's keep_handle): this object
        owns it from now on and destroys it."""
        self = cls.__new__(cls)
        self.lib, self.opts, self.desc_builder, self.hcap = lib, opts, None, 0
        self.h = C.c_void_p(handle)
        dims = (C.c_int64 * 6)()
        abi.check(self.lib, self.lib.tog_dims(self.h, dims))
        self.n, self.m, self.N, self.B, self.pmax, _ = [int(v) for v in dims]
        return self

    def __del__(self):
        try:
            if getattr(self, "h", None) is not None and self.h:
                self.lib.tog_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ shapes per field
    def shape(self, field):
        n, m, N, B, P = self.n, self.m, self.N, self.B, max(self.pmax, 1)
        return {
            abi.FIELD_X: (B, N, n), abi.FIELD_U: (B, N - 1, m), abi.FIELD_XBAR: (B, N, n),
            abi.FIELD_UBAR: (B, N - 1, m), abi.FIELD_K: (B, N - 1, n, m), abi.FIELD_D: (B, N - 1, m),
            abi.FIELD_A: (B, N - 1, n, n), abi.FIELD_B: (B, N - 1, m, n), abi.FIELD_S: (B, N, n, n),
            abi.FIELD_SX: (B, N, n), abi.FIELD_DV: (B, 2), abi.FIELD_LAMBDA: (B, N, P),
            abi.FIELD_MU: (B, N, P), abi.FIELD_C: (B, N, P), abi.FIELD_X0: (B, n),
            abi.FIELD_STATS: (B, abi.NSTATS), abi.FIELD_RHO: (B, 2),
            abi.FIELD_Q: (B, N, n + m + n * n + m * m + m * n),
        }[field]

    def get(self, field, raw=False):
        """Copy a field to the host. Matrices come back as (…, rows, cols) (the raw buffer is
        column-major per block, i.e. the transpose in numpy C order)."""
        out = np.empty(self.shape(field), dtype=np.float64)
        abi.check(self.lib, self.lib.tog_get(self.h, field, abi.as_dp(out)))
        if raw:
            return out
        if field in (abi.FIELD_K, abi.FIELD_A, abi.FIELD_B, abi.FIELD_S):
            return np.ascontiguousarray(np.swapaxes(out, -1, -2))
        return out

    def set(self, field, value):
        v = np.asarray(value, dtype=np.float64)
        if field in (abi.FIELD_K, abi.FIELD_A, abi.FIELD_B, abi.FIELD_S):
            v = np.swapaxes(v, -1, -2)
        v = np.ascontiguousarray(v.reshape(self.shape(field)))
        abi.check(self.lib, self.lib.tog_set(self.h, field, abi.as_dp(v)))

    def device_ptr(self, field) -> int:
        p = C.c_void_p()
        abi.check(self.lib, self.lib.tog_get_device_ptr(self.h, field, C.byref(p)))
        return int(p.value or 0)

    # ------------------------------------------------------------------ state
    def upload_state(self, prob):
        x0 = np.ascontiguousarray(prob.x0, dtype=np.float64)
        U = np.ascontiguousarray(prob._U, dtype=np.float64)
        X = np.ascontiguousarray(prob._X, dtype=np.float64)
        Xp = abi.as_dp(X) if np.isfinite(X).all() else C.cast(None, C.POINTER(C.c_double))
        if not np.isfinite(X).all() and not np.isnan(X).all():
            # a partially finite X0: upload as given (rollout!(prob) will trigger on the NaNs)
            Xp = abi.as_dp(X)
        abi.check(self.lib, self.lib.tog_set_state(self.h, abi.as_dp(x0), abi.as_dp(U), Xp))
        self.upload_trajectory_data(prob)

    # ------------------------------------------------------------------ per-trajectory costs and goals
    def upload_trajectory_data(self, prob):
        """The problem's BatchObjective tables and per-trajectory goals. A part the problem does not have goes
        back to the shared values if the handle holds a table for it (a handle that never held one is not
        touched)."""
        obj = getattr(prob, "obj", None)
        if hasattr(obj, "lin"):
            self.set_trajectory_costs(obj.lin, obj.term)
        elif getattr(self, "_traj_costs", False):
            self.set_trajectory_costs(None, None)
        goals = prob.trajectory_goals() if hasattr(prob, "trajectory_goals") else None
        if goals is not None:
            self.set_trajectory_goals(goals)
        elif getattr(self, "_traj_goals", False):
            self.set_trajectory_goals(None)
        obs = prob.trajectory_obstacles() if hasattr(prob, "trajectory_obstacles") else None
        if obs is not None:
            self.set_trajectory_obstacles(obs)
        elif getattr(self, "_traj_obstacles", False):
            self.set_trajectory_obstacles(None)
        bnd = prob.trajectory_bounds() if hasattr(prob, "trajectory_bounds") else None
        if bnd is not None:
            self.set_trajectory_bounds(bnd)
        elif getattr(self, "_traj_bounds", False):
            self.set_trajectory_bounds(None)
        W = prob.trajectory_weights() if hasattr(prob, "trajectory_weights") else None
        if W is not None:
            self.set_trajectory_weights(W)
        elif getattr(self, "_traj_weights", False):
            self.set_trajectory_weights(None)

    def set_trajectory_costs(self, lin=None, term=None):
        """tog_set_trajectory_costs. lin: (B, n+m+1) rows [q; r; c], or (B, N-1, n+m+1) with a row per stage
        knot; term: (B, n+1) rows [qf; cf]. None: that part stays shared (both None: the shared objective)."""
        n, m, N, B = self.n, self.m, self.N, self.B
        null = C.cast(None, C.POINTER(C.c_double))
        per_knot, lp, tp = 0, null, null
        if lin is not None:
            lin = np.ascontiguousarray(lin, dtype=np.float64)
            if lin.shape == (B, N - 1, n + m + 1):
                per_knot = 1
            elif lin.shape != (B, n + m + 1):
                raise ValueError(f"lin must be ({B}, {n + m + 1}) or ({B}, {N - 1}, {n + m + 1}), got {lin.shape}")
            lp = abi.as_dp(lin)
        if term is not None:
            term = np.ascontiguousarray(term, dtype=np.float64)
            if term.shape != (B, n + 1):
                raise ValueError(f"term must be ({B}, {n + 1}), got {term.shape}")
            tp = abi.as_dp(term)
        abi.check(self.lib, self.lib.tog_set_trajectory_costs(self.h, per_knot, lp, tp))
        self._traj_costs = lin is not None or term is not None

    def set_trajectory_goals(self, xf=None):
        """tog_set_trajectory_goals. xf: (B, ng) values of the terminal goal rows; None: the descriptor's."""
        if xf is None:
            abi.check(self.lib, self.lib.tog_set_trajectory_goals(self.h, C.cast(None, C.POINTER(C.c_double))))
            self._traj_goals = False
            return
        xf = np.ascontiguousarray(xf, dtype=np.float64)
        if xf.ndim != 2 or xf.shape[0] != self.B:
            raise ValueError(f"xf must be ({self.B}, ng), got {xf.shape}")
        abi.check(self.lib, self.lib.tog_set_trajectory_goals(self.h, abi.as_dp(xf)))
        self._traj_goals = True

    def set_trajectory_obstacles(self, obs=None):
        """tog_set_trajectory_obstacles. obs: (B, no, 4) rows [x0, y0, z0, r] of every circle and sphere in the
        ABI's ordinal order (Problem.trajectory_obstacles); None: the descriptor's."""
        if obs is None:
            abi.check(self.lib, self.lib.tog_set_trajectory_obstacles(self.h, C.cast(None, C.POINTER(C.c_double))))
            self._traj_obstacles = False
            return
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.ndim != 3 or obs.shape[0] != self.B or obs.shape[2] != 4:
            raise ValueError(f"obs must be ({self.B}, no, 4), got {obs.shape}")
        abi.check(self.lib, self.lib.tog_set_trajectory_obstacles(self.h, abi.as_dp(obs)))
        self._traj_obstacles = True

    def set_trajectory_bounds(self, bnd=None):
        """tog_set_trajectory_bounds. bnd: (B, nb) limits of every kept bound row in the ABI's ordinal order
        (Problem.trajectory_bounds); None: the descriptor's."""
        if bnd is None:
            abi.check(self.lib, self.lib.tog_set_trajectory_bounds(self.h, C.cast(None, C.POINTER(C.c_double))))
            self._traj_bounds = False
            return
        bnd = np.ascontiguousarray(bnd, dtype=np.float64)
        if bnd.ndim != 2 or bnd.shape[0] != self.B:
            raise ValueError(f"bnd must be ({self.B}, nb), got {bnd.shape}")
        abi.check(self.lib, self.lib.tog_set_trajectory_bounds(self.h, abi.as_dp(bnd)))
        self._traj_bounds = True

    def set_trajectory_weights(self, W=None):
        """tog_set_trajectory_weights. W: (B, nw) rows [Q; R; H; Qf], each matrix column-major with the compact
        n and m, nw = 2n² + m² + mn (Problem.trajectory_weights); None: the descriptor's Hessians."""
        if W is None:
            abi.check(self.lib, self.lib.tog_set_trajectory_weights(self.h, C.cast(None, C.POINTER(C.c_double))))
            self._traj_weights = False
            return
        n, m = self.n, self.m
        nw = 2 * n * n + m * m + m * n
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.shape != (self.B, nw):
            raise ValueError(f"W must be ({self.B}, {nw}), got {W.shape}")
        abi.check(self.lib, self.lib.tog_set_trajectory_weights(self.h, abi.as_dp(W)))
        self._traj_weights = True

    def download_state(self, prob):
        prob._X[...] = self.get(abi.FIELD_X)
        prob._U[...] = self.get(abi.FIELD_U)

    # ------------------------------------------------------------------ step level
    def rollout_open_loop(self):
        abi.check(self.lib, self.lib.tog_rollout_open_loop(self.h))

    def slack_controls(self):
        """``slack_controls(prob)`` into U[m+1:m+n] (infeasible handles, infeasible.jl:63-80)."""
        abi.check(self.lib, self.lib.tog_slack_controls(self.h))

    def cost_expansion(self, sqrt=False, al=False):
        """``cost_expansion!`` into FIELD_Q (ilqr_methods.jl:55-62)."""
        abi.check(self.lib, self.lib.tog_cost_expansion(self.h, int(sqrt), int(al)))

    def jacobians(self):
        abi.check(self.lib, self.lib.tog_jacobians(self.h))

    def update_constraints(self):
        abi.check(self.lib, self.lib.tog_update_constraints(self.h))

    def cost(self, al=False):
        J = np.empty(self.B)
        abi.check(self.lib, self.lib.tog_cost(self.h, int(al), abi.as_dp(J)))
        return J

    def backward_pass(self, sqrt=False, al=False, store_S=False):
        dV = np.empty((self.B, 2))
        abi.check(self.lib, self.lib.tog_backward_pass(self.h, int(sqrt), int(al),
                                                       abi.BP_STORE_S if store_S else 0, abi.as_dp(dV)))
        return dV

    def forward_pass(self, J_prev, al=False):
        Jp = np.ascontiguousarray(np.broadcast_to(np.asarray(J_prev, dtype=np.float64), (self.B,)))
        J = np.empty(self.B)
        abi.check(self.lib, self.lib.tog_forward_pass(self.h, int(al), abi.as_dp(Jp), abi.as_dp(J)))
        return J

    def rollout(self, alpha=1.0):
        ok = np.empty(self.B, dtype=np.int32)
        abi.check(self.lib, self.lib.tog_rollout(self.h, float(alpha), ok.ctypes.data_as(C.POINTER(C.c_int32))))
        return ok.astype(bool)

    # ------------------------------------------------------------------ solve level
    def solve_init(self, mode):
        abi.check(self.lib, self.lib.tog_solve_init(self.h, int(mode)))

    def solve_step(self, nsteps=1):
        abi.check(self.lib, self.lib.tog_solve_step(self.h, int(nsteps)))

    def solve_budget(self, mode):
        """tog_solve_budget: default batch-step budget of a solve to completion."""
        rc = self.lib.tog_solve_budget(self.h, int(mode))
        if rc <= 0:
            abi.check(self.lib, rc)
        return int(rc)

    def solve(self, mode, max_steps=None):
        """tog_solve; max_steps None/0: the tog_solve_budget default"""
        abi.check(self.lib, self.lib.tog_solve(self.h, int(mode), int(max_steps or 0)))

    # ------------------------------------------------------------------ streamed solves
    @staticmethod
    def _slots(slots):
        s = np.ascontiguousarray(np.asarray(slots, dtype=np.int32).ravel())
        return s, s.ctypes.data_as(C.POINTER(C.c_int32))

    def finished(self):
        """tog_finished: the slots whose trajectory finished and that were not listed before (ascending)."""
        out = np.empty(self.B, dtype=np.int32)
        cnt = C.c_int32()
        abi.check(self.lib, self.lib.tog_finished(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(cnt)))
        return out[:cnt.value].copy()

    def get_slots(self, field, slots):
        """tog_get_slots: tog_get's blocks of the listed slots, (count, ...) in list order (raw layout)."""
        s, sp = self._slots(slots)
        if field == abi.FIELD_HIST_INNER:
            shape = (self.hcap, 3)
        elif field == abi.FIELD_HIST_OUTER:
            shape = (self.opts.al_iterations + 1, 4)
        elif field == abi.FIELD_HIST_COUNT:
            shape = (2,)
        else:
            shape = self.shape(field)[1:]
        out = np.empty((len(s),) + tuple(shape), dtype=np.float64)
        abi.check(self.lib, self.lib.tog_get_slots(self.h, int(field), len(s), sp, abi.as_dp(out)))
        return out

    def refill(self, slots, x0, U, X=None):
        """tog_refill: start new trajectories in the listed (inactive) slots: x0 (count, n), U (count, N-1, m),
        X (count, N, n) or None (the initial rollout)."""
        s, sp = self._slots(slots)
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(len(s), self.n)
        U = np.ascontiguousarray(U, dtype=np.float64).reshape(len(s), self.N - 1, self.m)
        Xp = C.cast(None, C.POINTER(C.c_double))
        if X is not None:
            X = np.ascontiguousarray(X, dtype=np.float64).reshape(len(s), self.N, self.n)
            Xp = abi.as_dp(X)
        abi.check(self.lib, self.lib.tog_refill(self.h, len(s), sp, abi.as_dp(x0), abi.as_dp(U), Xp))

    def refill_tables(self, slots, lin=None, term=None, xf=None):
        """tog_refill_tables: the listed slots' rows of the per-trajectory tables the handle has."""
        s, sp = self._slots(slots)
        null = C.cast(None, C.POINTER(C.c_double))
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (lin, term, xf)]
        for a in arrs:
            if a is not None and a.shape[0] != len(s):
                raise ValueError("a table needs one row per listed slot")
        abi.check(self.lib, self.lib.tog_refill_tables(self.h, len(s), sp,
                                                       *[null if a is None else abi.as_dp(a) for a in arrs]))

    def solve_stream(self, mode, x0, U0, lin=None, term=None, xf=None, max_steps=None):
        """tog_solve_stream (tog_solve_stream_tables when any of lin, term, xf is given): the J jobs x0 (J, n),
        U0 (J, N-1, m) through this handle's B slots. Returns (X (J, N, n), U (J, N-1, m), stats (J, NSTATS),
        jobs_done)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        U0 = np.ascontiguousarray(U0, dtype=np.float64)
        J = x0.shape[0]
        if x0.shape != (J, self.n) or U0.shape != (J, self.N - 1, self.m):
            raise ValueError(f"x0 must be (J, {self.n}) and U0 (J, {self.N - 1}, {self.m})")
        X = np.zeros((J, self.N, self.n))
        U = np.zeros((J, self.N - 1, self.m))
        S = np.zeros((J, abi.NSTATS))
        done = C.c_int64()
        ms = int(max_steps or 0)
        if lin is None and term is None and xf is None:
            abi.check(self.lib, self.lib.tog_solve_stream(self.h, int(mode), J, abi.as_dp(x0), abi.as_dp(U0),
                                                          abi.as_dp(X), abi.as_dp(U), abi.as_dp(S), ms, C.byref(done)))
        else:
            null = C.cast(None, C.POINTER(C.c_double))
            arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (lin, term, xf)]
            for a in arrs:
                if a is not None and a.shape[0] != J:
                    raise ValueError("a table needs one row per job")
            abi.check(self.lib, self.lib.tog_solve_stream_tables(
                self.h, int(mode), J, abi.as_dp(x0), abi.as_dp(U0), *[null if a is None else abi.as_dp(a) for a in arrs],
                abi.as_dp(X), abi.as_dp(U), abi.as_dp(S), ms, C.byref(done)))
        return X, U, S, int(done.value)

    def solve_pn(self, pn_opts: abi.tog_pn_options):
        """tog_solve_pn: returns the (B, PN_NSTATS) statistics rows."""
        out = np.zeros((self.B, abi.PN_NSTATS))
        abi.check(self.lib, self.lib.tog_solve_pn(self.h, C.byref(pn_opts), abi.as_dp(out)))
        return out

    def batch_stats(self):
        out = np.empty(3)
        abi.check(self.lib, self.lib.tog_batch_stats(self.h, abi.as_dp(out)))
        return out

    def batch_stats_begin(self):
        """tog_batch_stats_begin: enqueue the stopping check (no host wait)."""
        abi.check(self.lib, self.lib.tog_batch_stats_begin(self.h))

    def batch_stats_end(self):
        """tog_batch_stats_end: wait for the enqueued check only; [n_active, Σ J, max c_max]."""
        out = np.empty(3)
        abi.check(self.lib, self.lib.tog_batch_stats_end(self.h, abi.as_dp(out)))
        return out

    def total_steps(self):
        v = C.c_int64()
        abi.check(self.lib, self.lib.tog_total_steps(self.h, C.byref(v)))
        return int(v.value)

    def profile(self, enable: bool):
        abi.check(self.lib, self.lib.tog_profile(self.h, int(bool(enable))))

    def profile_read(self):
        ms = np.zeros(abi.NKERNELS)
        cnt = (C.c_int64 * abi.NKERNELS)()
        abi.check(self.lib, self.lib.tog_profile_read(self.h, abi.as_dp(ms), cnt))
        return ms, np.array(list(cnt), dtype=np.int64)

    def rollout_plan(self, cnt=None, listed=False):
        """tog_rollout_plan: the rollout kernel (abi.ROLLOUT_*) a line-search launch of trials [0, cnt) takes on the
        handle's current flags; cnt None: every trial (iterations_linesearch + 1)."""
        if cnt is None:
            cnt = min(int(self.opts.iterations_linesearch) + 1, 64)
        k = C.c_int32()
        abi.check(self.lib, self.lib.tog_rollout_plan(self.h, int(cnt), int(bool(listed)), C.byref(k)))
        return int(k.value)

    def synchronize(self):
        abi.check(self.lib, self.lib.tog_synchronize(self.h))

    def status(self):
        f = np.empty(self.B, dtype=np.int32)
        abi.check(self.lib, self.lib.tog_status(self.h, f.ctypes.data_as(C.POINTER(C.c_int32))))
        return f

    def stats_dict(self):
        return stats_dict(self.get(abi.FIELD_STATS))

    # ------------------------------------------------------------------ iteration histories
    def enable_history(self, capacity: int):
        """tog_history_enable: keep `capacity` inner records per trajectory (0: off)."""
        abi.check(self.lib, self.lib.tog_history_enable(self.h, int(capacity)))
        self.hcap = int(capacity)

    def history(self):
        """(inner (B, cap, 3) [cost, dJ, gradient], outer (B, al_iterations + 1, 4) [iterations_inner, cost,
        c_max, penalty_max], counts (B, 2) records written [inner, outer]) of the solve since
        tog_solve_init; None when recording is off."""
        if not self.hcap:
            return None
        inner = np.empty((self.B, self.hcap, 3))
        abi.check(self.lib, self.lib.tog_get(self.h, abi.FIELD_HIST_INNER, abi.as_dp(inner)))
        ocap = self.opts.al_iterations + 1
        outer = np.empty((self.B, ocap, 4))
        abi.check(self.lib, self.lib.tog_get(self.h, abi.FIELD_HIST_OUTER, abi.as_dp(outer)))
        cnt = np.empty((self.B, 2))
        abi.check(self.lib, self.lib.tog_get(self.h, abi.FIELD_HIST_COUNT, abi.as_dp(cnt)))
        return inner, outer, cnt.astype(np.int64)

    def pn_history(self, n_steps: int):
        """solver_pn.stats [:cost, :c_max] per newton step (B, n_steps, 2) and records per trajectory (B,)."""
        out = np.empty((self.B, max(int(n_steps), 0), 2))
        rec = np.zeros(self.B, dtype=np.int32)
        abi.check(self.lib, self.lib.tog_get_pn_history(self.h, abi.as_dp(out), rec.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, rec


def stats_dict(S):
    """solver.stats from the (B, TOG_NSTATS) statistics rows (TOG_FIELD_STATS)."""
    return {
        "cost": S[:, abi.STAT_J], "dJ": S[:, abi.STAT_DJ], "gradient": S[:, abi.STAT_GRADIENT],
        "iterations": S[:, abi.STAT_ITERATIONS].astype(np.int64),
        "dJ_zero_counter": S[:, abi.STAT_ZERO_COUNT].astype(np.int64),
        "alpha": S[:, abi.STAT_ALPHA], "c_max": S[:, abi.STAT_C_MAX],
        "iterations_outer": S[:, abi.STAT_AL_ITER].astype(np.int64),
        "iterations_total": S[:, abi.STAT_TOTAL_STEPS].astype(np.int64),
        "penalty_max": S[:, abi.STAT_PENALTY_MAX],
        "flags": S[:, abi.STAT_FLAGS].astype(np.int64),
    }


def ilqr_traj_stats(inner, n_rec, zero_counter=None):
    """One inner solve's ``solver.stats`` as iLQRSolver's record_iteration! builds it (ilqr_methods.jl:77-89):
    :iterations, and the :cost, :dJ, :gradient vectors; `inner` holds its records."""
    d = {"iterations": int(n_rec), "cost": inner[:n_rec, 0].copy(), "dJ": inner[:n_rec, 1].copy(),
         "gradient": inner[:n_rec, 2].copy()}
    if zero_counter is None:  # dJ == 0 counts consecutive records (the counter's value after the last one)
        z = 0
        for v in d["dJ"]:
            z = z + 1 if v == 0.0 else 0
        zero_counter = z
    d["dJ_zero_counter"] = int(zero_counter)
    return d


def al_traj_stats(inner, n_in, outer, n_out):
    """AugmentedLagrangianSolver.stats of one trajectory (augmented_lagrangian_methods.jl:79-97):
    :iterations, :iterations_total, the :iterations_inner, :cost, :c_max, :penalty_max vectors, and
    stats_uncon (the inner solver's stats at every outer record; the first is the reset solver's). The
    inner records are split by :iterations_inner; records past the history's capacity are absent, so a
    truncated history leaves the later inner solves short."""
    it_in = outer[:n_out, 0].astype(np.int64)
    d = {"iterations": int(n_out), "iterations_total": int(it_in.sum()), "iterations_inner": it_in,
         "cost": outer[:n_out, 1].copy(), "c_max": outer[:n_out, 2].copy(), "penalty_max": outer[:n_out, 3].copy()}
    inner = inner[:min(int(n_in), inner.shape[0])]
    uncon, o = [], 0
    for k in it_in:
        sl = inner[o:o + int(k)]
        uncon.append(ilqr_traj_stats(sl, len(sl)))
        o += int(k)
    d["stats_uncon"] = uncon
    d["truncated"] = bool(n_in > inner.shape[0])
    return d

