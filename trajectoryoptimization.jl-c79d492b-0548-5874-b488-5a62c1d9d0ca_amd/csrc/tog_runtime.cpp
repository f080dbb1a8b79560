// tog_runtime.cpp — C ABI (include/tog.h) over the HIP kernels. Host code only: device buffers,
// problem marshalling (tog_problem_desc -> DevProblem + constraint rows), launch sequencing.
//
// Ownership: the handle owns every device buffer; callers own host arrays. One host thread per
// handle; handles are independent (one per GPU for multi-GPU runs).
#include <cmath>
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <chrono>
#include <thread>
#include <vector>

#include <dlfcn.h>

#include "tog_plugin.hpp"
#include "tog_host_plan.hpp"
#include "tog_traj_tables.hpp"
#include "tog_stream.hpp"
#include "tog_cost_plugin.hpp"

using namespace tog;

// The built-in models: X(model id, unit suffix). Each has four translation units, k_<suffix>.hip (ops_<suffix>),
// k_inf_<suffix>.hip (add_slack_controls(model): infeasible start, src/model.jl:761-779), k_mt_<suffix>.hip
// (add_min_time_controls(model): minimum time, src/solvers/altro/minimum_time.jl:83-104) and k_mtinf_<suffix>.hip
// (minimum_time_problem(infeasible_problem(prob))).
#define TOG_BUILTIN_MODELS(X)                        \
  X(TOG_MODEL_DOUBLE_INTEGRATOR, double_integrator)  \
  X(TOG_MODEL_CARTPOLE, cartpole)                    \
  X(TOG_MODEL_QUADROTOR, quadrotor)                  \
  X(TOG_MODEL_CAR, car)                              \
  X(TOG_MODEL_PENDULUM, pendulum)                    \
  X(TOG_MODEL_KUKA, kuka)

namespace tog {
#define X(id, unit)                  \
  const ModelOps* ops_##unit();      \
  const ModelOps* ops_inf_##unit();  \
  const ModelOps* ops_mt_##unit();   \
  const ModelOps* ops_mtinf_##unit();
TOG_BUILTIN_MODELS(X)
#undef X
const ModelOps* ops_kuka_implicit();  // the Kuka under the implicit integrators (k_kuka_implicit.hip)
}  // namespace tog

static thread_local std::string g_err;

// active trajectories at or below which tog_solve_step runs the latency-sized kernel variants
// (DevBuffers::tail): 2048 trajectories = 512 team waves, at most one per SIMD
static constexpr double TAIL_ACTIVE = 2048.0;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// Host watchdog of the blocking readbacks: wait for `ev` polling, and give up after TOG_WATCHDOG_S seconds
// (default 600) with TOG_ERR_DEVICE, so that a kernel that never finishes (e.g. a lost LDS hand-off in the
// tail backward kernel, whose waits are unbounded for speed, tog_bwd_quad.hpp) is reported instead of
// blocking the caller forever. The device queue itself stays hung: the process should exit.
static int wait_event(hipEvent_t ev, const char* what) {
  static const double limit = getenv("TOG_WATCHDOG_S") ? atof(getenv("TOG_WATCHDOG_S")) : 600.0;
  const auto t0 = std::chrono::steady_clock::now();
  unsigned polls = 0;
  while (true) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return TOG_OK;
    if (e != hipErrorNotReady) return fail(TOG_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    if (++polls > 64) {  // (first a short spin: a check usually completes within microseconds)
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit)
        return fail(TOG_ERR_DEVICE, std::string(what) + ": the device did not finish within TOG_WATCHDOG_S = " +
                                        std::to_string(limit) + " s (a hung kernel?)");
      std::this_thread::sleep_for(std::chrono::microseconds(polls < 1000 ? 2 : 200));
    }
  }
}

#define HIPCHECK(expr)                                                                   \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) return fail(TOG_ERR_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

struct tog_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int model = 0, integ = 0, n = 0, m = 0, N = 0, pmax = 0, nrows = 0, nq = 0;
  long long B = 0;
  double last_active = -1.0;  // n_active of the last host stats readback (-1: none yet)
  int mode = TOG_MODE_ILQR;
  tog_options opts;
  DevProblem hostP;
  DevProblem* dP = nullptr;
  int* d_knot_off = nullptr;
  int* d_knot_cnt = nullptr;
  int* d_knot_nx = nullptr;
  ConRow* d_rows = nullptr;
  DevBuffers buf = {};
  const ModelOps* ops = nullptr;
  int bwd_team = 0;  // backward pass on column-per-lane teams (else one wave per trajectory, LDS)
  double* d_scratch = nullptr;  // B doubles (J_prev / J_out staging)
  double* d_scratch2 = nullptr; // B doubles
  int* d_iscratch = nullptr;    // B ints
  double* d_stats = nullptr;    // 3 doubles
  int* d_act_list = nullptr;    // B ints: the active trajectories of a compacted tail step
  int* d_act_count = nullptr;
  std::vector<void*> allocs;
  // live per-kernel timing (tog_profile)
  bool profiling = false;
  std::vector<hipEvent_t> ev_pool;
  std::vector<int> ev_kind;  // kernel id per recorded (start, end) pair
  size_t ev_used = 0;
  // tog_create_multi: a handle over several devices owns one plain handle per device, each with a
  // contiguous slice [part_off[i], part_off[i+1]) of the batch; every entry point fans out
  std::vector<tog_handle*> parts;
  std::vector<long long> part_off;
  // second stream + fork/join events: the forward pass overlaps the decided trajectories' commit
  // with the second speculative round (tog_launch.hpp forward_i)
  StreamPair sp = {nullptr, nullptr, nullptr};
  // projected Newton workspace, allocated by the first tog_solve_pn (tog_pn.hpp)
  PNBuffers pn = {};
  bool pn_alloc = false, pn_opt_alloc = false;
  // a problem whose blocks can outgrow the narrow stride (n + pmax > 64): X, U as tog_solve_pn found them, for
  // the wide pass's restart; each trajectory's wide slot (-1: none) and its parked active flag
  double *pn_X0 = nullptr, *pn_U0 = nullptr;
  int *pn_slot_of = nullptr, *pn_park = nullptr;
  // solver_pn.stats histories of the last tog_solve_pn: (2, n_steps, B) [cost, c_max], records per trajectory
  std::vector<double> pn_hist;
  std::vector<int32_t> pn_hist_rec;
  int pn_hist_steps = -1;
  // asynchronous stopping check (tog_batch_stats_begin / _end): pinned landing buffer + completion event
  double* h_stats = nullptr;
  hipEvent_t stats_ev = nullptr;
  bool stats_pending = false;
  // tog_history_enable's allocations (DevBuffers::hist_in / hist_out point into them while recording is on)
  double *hist_in_alloc = nullptr, *hist_out_alloc = nullptr;
  int hist_cap_alloc = 0, hist_ocap_alloc = 0;
  hipEvent_t sync_ev = nullptr;  // tog_synchronize's watchdog wait
  // per-trajectory cost terms and goals (tog_set_trajectory_costs / _goals; DevProblem::lin, term, goal): the
  // device tables (null: the shared values), the per-knot cost table the descriptor came with (null: one stage
  // cost, whose table row is kc_row and whose N - 1 copies are d_kc_rep once a table is set) and its variant flag
  double *d_lin = nullptr, *d_term = nullptr, *d_goal = nullptr, *d_kc_rep = nullptr;
  const double* kc0 = nullptr;
  int tv0 = 0;
  std::vector<double> kc_row;
  std::vector<int> goal_idx;  // state index of each terminal goal row, in row order (ng = size)
  std::string goal_err;       // why the problem's goal rows cannot vary per trajectory (empty: they can)
  // per-trajectory obstacles (tog_set_trajectory_obstacles; DevProblem::obs): the device table (4, no, B), and
  // circle (0) or sphere (1) of each obstacle ordinal of the descriptor's sets table (no = size)
  double* d_obs = nullptr;
  std::vector<char> obs_kind;
  // per-trajectory bounds (tog_set_trajectory_bounds; DevProblem::bnd): the device table (nb, B), and per bound-row
  // ordinal of the descriptor's sets table whether its constraint is trimmed (nb = size)
  double* d_bnd = nullptr;
  std::vector<char> bnd_trimmed;
  // per-trajectory cost weights (tog_set_trajectory_weights; DevProblem::hess): the device table (nh, B), the
  // batch's sqrt_ok and diagonal-cost class while it is set, and the descriptor's, which clearing it restores
  double* d_hess = nullptr;
  int hess_sqrt_ok = 1, hess_diag = 0, sqrt_ok0 = 0, diag0 = 0;
  // Streamed solves (tog_finished / tog_get_slots / tog_refill / tog_solve_stream), allocated on first use and
  // freed in tog_destroy; everything is ordered on the handle's stream.
  // d_slot_job (B): the job a slot holds whose end has not been listed yet (-1: empty, or listed by
  // k_list_finished); d_fin (1 + B): k_list_finished's count and list; d_gl, d_rl (B each): the slot lists of a
  // gather and of a refill; h_ints: their pinned host images [fin (1 + B) | gl (B) | rl (B) | jobs (B)].
  int *d_slot_job = nullptr, *d_fin = nullptr, *d_gl = nullptr, *d_rl = nullptr, *d_rjob = nullptr, *h_ints = nullptr;
  // staging, a pinned host buffer and its device twin each, grown on demand: refill inputs (x0, U, X, the table
  // rows) and gathered results
  struct Stage {
    double *h = nullptr, *d = nullptr;
    size_t cap = 0;
  };
  Stage sin_x0, sin_U, sin_X, sin_tab, sout;
  hipEvent_t fin_ev = nullptr, refill_ev = nullptr, gather_ev = nullptr;
  bool refill_pending = false;
  long long jobs_started = 0;  // tog_refill's running job index
};

static hipEvent_t next_event(tog_handle* h) {
  if (h->ev_used == h->ev_pool.size()) {
    hipEvent_t e;
    (void)hipEventCreate(&e);
    h->ev_pool.push_back(e);
  }
  return h->ev_pool[h->ev_used++];
}

// launch `fn` bracketed by timing events when profiling is on
template <class F>
static void timed(tog_handle* h, int kind, F&& fn) {
  if (!h->profiling) {
    fn();
    return;
  }
  hipEvent_t a = next_event(h), b = next_event(h);
  (void)hipEventRecord(a, h->stream);
  fn();
  (void)hipEventRecord(b, h->stream);
  h->ev_kind.push_back(kind);
}

// a loaded GenericCost plugin (tog_generic_cost_load)
struct tog_generic_cost {
  using expand_fn = int (*)(int, const double*, const double*, long long, double*, double*, double*, double*,
                            double*, double*, void*);
  void* so;
  int n, m;
  expand_fn ex;
};

// a loaded user model plugin (tog_model_load)
struct tog_model {
  void* so;
  const tog::ModelOps* ops;
  const tog::ModelOps* ops_inf;
  const tog::ModelOps* ops_mt;  // MinTime<M> (add_min_time_controls)
};

// the built-in models' tables: at[variant: bit 0 infeasible, bit 1 minimum time][model id]
struct BuiltinOps {
  using fn = const ModelOps* (*)();
  fn at[4][TOG_MODEL_COUNT];
};
static BuiltinOps builtin_ops() {
  BuiltinOps t = {};
#define X(id, unit)              \
  t.at[0][id] = ops_##unit;      \
  t.at[1][id] = ops_inf_##unit;  \
  t.at[2][id] = ops_mt_##unit;   \
  t.at[3][id] = ops_mtinf_##unit;
  TOG_BUILTIN_MODELS(X)
#undef X
  return t;
}

static const ModelOps* ops_for(int model, bool infeasible, bool min_time, const tog_model* user, int integ) {
  if (model == TOG_MODEL_KUKA && !infeasible && !min_time && (integ == TOG_RK3_IMPLICIT || integ == TOG_MIDPOINT_IMPLICIT))
    return ops_kuka_implicit();
  if (model == TOG_MODEL_USER) {  // (a plugin has no minimum-time variant of its infeasible model)
    if (!user || (min_time && infeasible)) return nullptr;
    return min_time ? user->ops_mt : infeasible ? user->ops_inf : user->ops;
  }
  if (model < 0 || model >= TOG_MODEL_COUNT) return nullptr;
  static const BuiltinOps table = builtin_ops();
  const BuiltinOps::fn f = table.at[(min_time ? 2 : 0) | (infeasible ? 1 : 0)][model];
  return f ? f() : nullptr;
}

// Flatten the ordered constraint sets into per-knot rows (src/constraint_sets.jl:64-131).
static int build_rows(const tog_problem_desc* d, int slack, int pcap, int has_con, std::vector<ConRow>& rows,
                      std::vector<int>& off, std::vector<int>& cnt, std::vector<char>* obs_kind = nullptr,
                      std::vector<char>* bnd_trimmed = nullptr) {
  const int n = d->n, m = d->m, N = d->N;
  const int mt = (d->flags & TOG_PROB_MIN_TIME) ? 1 : 0;  // h, the last control
  off.assign(N, 0);
  cnt.assign(N, 0);
  // the ordinal of every circle and sphere (tog_set_trajectory_obstacles' table index, kept in ConRow::idx)
  std::vector<int> set_first(d->n_sets > 0 ? d->n_sets : 0, 0), obs_base;
  tog_traj::BoundPlan bplan;
  {
    std::vector<int> ncon, ctype, ccount;
    std::vector<const double*> cdata;
    for (int s = 0; s < d->n_sets; s++) {
      set_first[s] = (int)ctype.size();
      ncon.push_back(d->sets[s].n_con);
      for (int c = 0; c < d->sets[s].n_con; c++) {
        ctype.push_back(d->sets[s].con[c].type);
        ccount.push_back(d->sets[s].con[c].count);
        cdata.push_back(d->sets[s].con[c].data);
      }
    }
    std::vector<char> kind;
    tog_traj::obstacle_ordinals(ncon.data(), d->n_sets, ctype.data(), ccount.data(), TOG_CON_CIRCLES, TOG_CON_SPHERES,
                                obs_base, kind);
    if (obs_kind) *obs_kind = kind;
    // the ordinal of every kept bound row (tog_set_trajectory_bounds' table index, kept in ConRow::b, which no
    // reader of a bound row uses: DESIGN.md §8). A set that only the terminal knot uses has no control rows.
    std::vector<char> set_term(d->n_sets > 0 ? d->n_sets : 0, 0);
    if (d->knot_set && N > 0 && d->knot_set[N - 1] >= 0 && d->knot_set[N - 1] < d->n_sets) {
      set_term[d->knot_set[N - 1]] = 1;
      for (int k = 0; k < N - 1; k++)
        if (d->knot_set[k] == d->knot_set[N - 1]) set_term[d->knot_set[N - 1]] = 0;
    }
    tog_traj::bound_ordinals(ncon.data(), set_term.data(), d->n_sets, ctype.data(), ccount.data(), cdata.data(),
                             TOG_CON_BOUND, n, m, slack, mt, bplan);
    if (bnd_trimmed) *bnd_trimmed = bplan.trimmed;
  }
  for (int k = 0; k < N; k++) {
    off[k] = (int)rows.size();
    const int si = d->knot_set ? d->knot_set[k] : -1;
    if (si < 0) continue;
    if (si >= d->n_sets) return fail(TOG_ERR_ARG, "knot_set index out of range");
    const bool term = (k == N - 1);
    const tog_constraint_set& set = d->sets[si];
    for (int c = 0; c < set.n_con; c++) {
      const tog_constraint& con = set.con[c];
      const double* D = con.data;
      switch (con.type) {
        case TOG_CON_BOUND: {
          // data = [x_max(n), x_min(n), u_max(m), u_min(m)]; order [x_max; u_max; x_min; u_min].
          // count 0: trim = true (infinite bounds dropped); 1: trim = false (every row kept). The slack
          // controls of an infeasible-start problem are never bounded: its BoundConstraint keeps the model's
          // m (update_constraint_set_jacobians, constraint_sets.jl:135-150)
          // (trimmed bounds: rows for the finite entries over all m; the infeasible minimum-time problem's
          // combined bound reaches u[1:m+1], mintime_constraints, minimum_time.jl:125-141)
          // (trim=false: the model's controls and, on a minimum-time problem, the time step h = u[m-1])
          const bool keep = (con.count == 1);
          auto u_row = [&](int i) { return tog_traj::bound_u_kept(i, keep, m, slack, mt); };
          // (ord: the row's ordinal, counted from its block's first over the kept rows; the x blocks of a set
          // that stage knots and the terminal knot share keep the stage rows' ordinals)
          const int* ob = &bplan.base[4 * (size_t)(set_first[si] + c)];
          int ord = ob[0];
          for (int i = 0; i < n; i++)
            if (keep || isfinite(D[i])) rows.push_back({ROW_XMAX, i, D[i], (double)ord++, 0, 0});
          ord = ob[1];
          if (!term)
            for (int i = 0; i < m; i++)
              if (u_row(i) && (keep || isfinite(D[2 * n + i]))) rows.push_back({ROW_UMAX, i, D[2 * n + i], (double)ord++, 0, 0});
          ord = ob[2];
          for (int i = 0; i < n; i++)
            if (keep || isfinite(D[n + i])) rows.push_back({ROW_XMIN, i, D[n + i], (double)ord++, 0, 0});
          ord = ob[3];
          if (!term)
            for (int i = 0; i < m; i++)
              if (u_row(i) && (keep || isfinite(D[2 * n + m + i]))) rows.push_back({ROW_UMIN, i, D[2 * n + m + i], (double)ord++, 0, 0});
          break;
        }
        case TOG_CON_GOAL: {  // count: rows x[1:count] - xf (the goal's inds); 0 = n
          const int ng = con.count > 0 ? con.count : n;
          if (ng > n) return fail(TOG_ERR_ARG, "goal constraint longer than the state");
          if (term)
            for (int i = 0; i < ng; i++) rows.push_back({ROW_GOAL, i, D[i], 0, 0, 0});
          break;
        }
        case TOG_CON_CIRCLES:
          if (!term)
            for (int o = 0; o < con.count; o++)
              rows.push_back({ROW_CIRCLE, obs_base[set_first[si] + c] + o, D[3 * o], D[3 * o + 1], 0.0, D[3 * o + 2]});
          break;
        case TOG_CON_SPHERES:
          if (!term)
            for (int o = 0; o < con.count; o++)
              rows.push_back({ROW_SPHERE, obs_base[set_first[si] + c] + o, D[4 * o], D[4 * o + 1], D[4 * o + 2], D[4 * o + 3]});
          break;
        case TOG_CON_INFEASIBLE:
          // infeasible_constraints(n, m) (src/constraints.jl:306-314): c = u[m+1:m+n], stage only
          if (!slack) return fail(TOG_ERR_ARG, "TOG_CON_INFEASIBLE needs a TOG_PROB_INFEASIBLE problem");
          if (!term)
            for (int i = 0; i < slack; i++) rows.push_back({ROW_USLACK, m - slack - mt + i, 0.0, 0.0, 0.0, 0.0});
          break;
        case TOG_CON_MIN_TIME_EQ:
          if (!(d->flags & TOG_PROB_MIN_TIME)) return fail(TOG_ERR_ARG, "TOG_CON_MIN_TIME_EQ needs a TOG_PROB_MIN_TIME problem");
          if (!term) rows.push_back({ROW_MT_EQ, n - 1, (double)(m - 1), 0.0, 0.0, 0.0});
          break;
        case TOG_CON_USER: {
          if (!has_con) return fail(TOG_ERR_ARG, "TOG_CON_USER needs a user model plugin that defines con()");
          const int where = (int)D[2];
          if (con.count < 1 || con.count > PUSER) return fail(TOG_ERR_ARG, "user constraint: 1 <= p <= 16");
          if ((term && where != 0) || (!term && where != 1))
            for (int i = 0; i < con.count; i++)
              rows.push_back({D[1] != 0.0 ? ROW_USER_EQ : ROW_USER_INEQ, i, D[0], (double)con.count, 0.0, 0.0});
          break;
        }
        default:
          return fail(TOG_ERR_ARG, "unknown constraint type");
      }
    }
    cnt[k] = (int)rows.size() - off[k];
    if (cnt[k] > pcap) return fail(TOG_ERR_UNSUPPORTED, "too many constraint rows at one knot (PCAP)");
    // knots with the same rows share one copy (stage knots of one ConstraintSet): the table stays
    // small enough for the backward kernel to cache it in LDS
    for (int j = 0; j < k; j++) {
      if (cnt[j] != cnt[k] || cnt[k] == 0) continue;
      if (memcmp(&rows[off[j]], &rows[off[k]], sizeof(ConRow) * cnt[k]) == 0) {
        rows.resize(off[k]);
        off[k] = off[j];
        break;
      }
    }
  }
  return TOG_OK;
}

template <class T>
static int dalloc(tog_handle* h, T** p, size_t count) {
  void* v = nullptr;
  HIPCHECK(hipMalloc(&v, count * sizeof(T) > 0 ? count * sizeof(T) : 16));
  h->allocs.push_back(v);
  *p = (T*)v;
  return TOG_OK;
}
// release one dalloc'ed buffer before the handle is destroyed (null: nothing)
static void dfree(tog_handle* h, void* v) {
  if (!v) return;
  for (size_t i = 0; i < h->allocs.size(); i++)
    if (h->allocs[i] == v) {
      (void)hipFree(v);
      h->allocs.erase(h->allocs.begin() + (long)i);
      return;
    }
}

// =============================================================================================
// k_batch_stats: [n_active, Σ J, max c_max] (input to the cross-GPU RCCL all-reduce)
// =============================================================================================
static __global__ void __launch_bounds__(1024) k_batch_stats(const TrajState* __restrict__ st, long long B, double* out) {
  __shared__ double sa[1024], sj[1024], sc[1024];
  const int t = threadIdx.x;
  double a = 0.0, j = 0.0, c = 0.0;
  for (long long b = t; b < B; b += blockDim.x) {
    a += st[b].active ? 1.0 : 0.0;
    j += st[b].J;
    c = tog_jlmax(c, st[b].c_max);  // a NaN violation propagates (Julia max), never reads as feasible
  }
  sa[t] = a;
  sj[t] = j;
  sc[t] = c;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if (t < w) {
      sa[t] += sa[t + w];
      sj[t] += sj[t + w];
      sc[t] = tog_jlmax(sc[t], sc[t + w]);
    }
    __syncthreads();
  }
  if (t == 0) {
    out[0] = sa[0];
    out[1] = sj[0];
    out[2] = sc[0];
  }
}


// the active trajectories, for the compacted launches of a tail step (order immaterial: every
// trajectory's computation is independent of its slot)
static __global__ void __launch_bounds__(256) k_list_active(const TrajState* __restrict__ st, long long B, int* list,
                                                            int* count) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool a = b < B && st[b].active;
  const unsigned long long mask = __ballot(a);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(count, __popcll(mask));
  base = __shfl(base, leader);
  if (a) list[base + __popcll(mask & ((1ull << lane) - 1))] = (int)b;
}

// Streamed solves: the slots that hold a job (slot_job >= 0), are inactive and were not listed before, compacted
// as k_list_active does; a listed slot is marked (slot_job = -1), so every finished job is listed once. out[0] is
// the count, out + 1 the list.
static __global__ void __launch_bounds__(256) k_list_finished(const TrajState* __restrict__ st, int* slot_job,
                                                              long long B, int* out) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool f = b < B && slot_job[b] >= 0 && !st[b].active;
  const unsigned long long mask = __ballot(f);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(out, __popcll(mask));
  base = __shfl(base, leader);
  if (f) {
    out[1 + base + __popcll(mask & ((1ull << lane) - 1))] = (int)b;
    slot_job[b] = -1;
  }
}

// slot_job[b] = b: every slot holds the trajectory tog_solve_init started in it
static __global__ void k_slot_iota(int* slot_job, long long B) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) slot_job[b] = (int)b;
}
// every slot empty and inactive (the start of a streamed solve)
static __global__ void k_slots_clear(TrajState* st, int* slot_job, long long B) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  st[b].active = 0;
  slot_job[b] = -1;
}
// the listed slots hold these jobs from now on (after k_refill)
static __global__ void k_slots_mark(int* slot_job, const int* __restrict__ list, const int* __restrict__ jobs,
                                    int count, long long B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int b = list[i];
  if (b >= 0 && b < B) slot_job[b] = jobs[i];
}

// A field's blocks (w doubles per slot) of the listed slots into a contiguous buffer, block i = slot list[i];
// one workgroup per listed slot, lanes over the block's entries (coalesced both ways). k_scatter_slots is the
// inverse (the table rows of a refill).
static __global__ void __launch_bounds__(256) k_gather_slots(const double* __restrict__ src, size_t w,
                                                             const int* __restrict__ list, long long B,
                                                             double* __restrict__ dst) {
  const long long b = list[blockIdx.x];
  if (b < 0 || b >= B) return;
  const double* s = src + (size_t)b * w;
  double* d = dst + (size_t)blockIdx.x * w;
  for (size_t e = threadIdx.x; e < w; e += blockDim.x) d[e] = s[e];
}
static __global__ void __launch_bounds__(256) k_scatter_slots(double* __restrict__ dst, size_t w,
                                                              const int* __restrict__ list, long long B,
                                                              const double* __restrict__ src) {
  const long long b = list[blockIdx.x];
  if (b < 0 || b >= B) return;
  const double* s = src + (size_t)blockIdx.x * w;
  double* d = dst + (size_t)b * w;
  for (size_t e = threadIdx.x; e < w; e += blockDim.x) d[e] = s[e];
}

__global__ void k_fill(double* p, size_t count, double v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) p[i] = v;
}

static void fill(tog_handle* h, double* p, size_t count, double v) {
  if (!count) return;
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, p, count, v);
}

__global__ void k_reset_state(TrajState* st, long long B, double mu0) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  TrajState s = {};
  s.active = 1;
  (void)mu0;
  st[b] = s;
}

// Projected Newton's wide pass (tog_solve_pn), a workgroup per trajectory. enter: a trajectory with a slot
// goes back to the X, U the call started from, without the narrow pass's flags; every other one is parked
// (k_jacobian skips it, so nothing of it moves). leave: the parked ones get their active flag back.
static __global__ void __launch_bounds__(64) k_pn_wide_gate(TrajState* st, const int* __restrict__ slot_of, int* park,
                                                            double* X, double* U, const double* __restrict__ X0,
                                                            const double* __restrict__ U0, long long nx, long long nu,
                                                            int enter) {
  const long long b = blockIdx.x;
  if (slot_of[b] < 0) {
    if (threadIdx.x == 0) {
      if (enter) {
        park[b] = st[b].active;
        st[b].active = 0;
      } else {
        st[b].active = park[b];
      }
    }
  } else if (enter) {
    for (long long e = threadIdx.x; e < nx; e += 64) X[b * nx + e] = X0[b * nx + e];
    for (long long e = threadIdx.x; e < nu; e += 64) U[b * nu + e] = U0[b * nu + e];
    if (threadIdx.x == 0) st[b].flags &= ~(TOG_TRAJ_PN_ERROR | TOG_TRAJ_PN_BLOCK);
  }
}

// The host loop of solve!(prob, ProjectedNewtonSolver) over one workspace (tog_solve_pn): `launch(phase)` runs a
// phase's kernel over the workspace's `cnt` workgroups, workgroup s solving trajectory traj(s). Fills the
// trajectories' pn_hist rows; `stp` returns the states after the last newton step.
template <class Launch, class Traj>
static int32_t pn_pass(tog_handle* h, const tog_pn_options* opts, bool optimal, const PNState* d_st, long long cnt,
                       std::vector<PNState>& stp, Launch&& launch, Traj&& traj) {
  const long long B = h->B;
  int32_t rc;
  auto run = [&](int phase) -> int32_t {
    const hipError_t e = (hipError_t)launch(phase);
    if (e != hipSuccess)
      return fail(TOG_ERR_DEVICE, std::string("projected Newton: the kernel's LDS limit could not be raised: ") + hipGetErrorString(e));
    return TOG_OK;
  };
  stp.assign(cnt, PNState{});
  for (int step = 0; step < opts->n_steps; step++) {
    if ((rc = run(0))) return rc;
    for (int it = 0; it < 10; it++) {
      h->ops->jacobian(h->dP, h->buf, B, h->N, h->integ, h->stream);
      if ((rc = run(1))) return rc;
    }
    if (optimal) {  // the KKT step and its line search: 10 trials of at most 12 projection! passes
      if ((rc = run(3))) return rc;
      h->ops->jacobian(h->dP, h->buf, B, h->N, h->integ, h->stream);
      if ((rc = run(4))) return rc;
      for (int ls = 0; ls < 10; ls++) {
        for (int it = 0; it < 12; it++) {
          h->ops->jacobian(h->dP, h->buf, B, h->N, h->integ, h->stream);
          if ((rc = run(5))) return rc;
        }
        if ((rc = run(6))) return rc;
      }
    }
    if ((rc = run(2))) return rc;
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(stp.data(), d_st, sizeof(PNState) * cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    for (long long s = 0; s < cnt; s++)
      if (stp[s].steps == step + 1) {
        const size_t b = (size_t)traj(s);
        h->pn_hist[2 * (b * opts->n_steps + step)] = stp[s].J;
        h->pn_hist[2 * (b * opts->n_steps + step) + 1] = stp[s].c_max;
      }
  }
  return TOG_OK;
}

// the device's LDS a workgroup may ask for (gfx950: 160 KB), for the check of a projected Newton path's need
static int32_t pn_lds_limit(tog_handle* h, size_t* out) {
  int optin = 0, plain = 0;
  HIPCHECK(hipDeviceGetAttribute(&plain, hipDeviceAttributeMaxSharedMemoryPerBlock, h->device));
  // (what a kernel may opt into, where the runtime reports it apart from the plain limit)
  if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, h->device) != hipSuccess) {
    (void)hipGetLastError();
    optin = 0;
  }
  *out = (size_t)std::max(optin, plain);
  return TOG_OK;
}

// device buffers of one call, released when it returns
struct ScopedDev {
  std::vector<void*> p;
  ~ScopedDev() {
    for (void* v : p) (void)hipFree(v);
  }
  template <class T>
  hipError_t get(T** out, size_t count) {
    void* v = nullptr;
    const hipError_t e = hipMalloc(&v, count * sizeof(T) > 0 ? count * sizeof(T) : 16);
    if (e == hipSuccess) p.push_back(v);
    *out = (T*)v;
    return e;
  }
};

// tog_solve_pn's second pass: the trajectories `trajs`, whose blocks outgrew the narrow stride, are solved again
// from the call's starting point with the wide kernels (tog_pn.hpp) in a workspace of trajs.size() slots. Their
// pn_hist rows are rewritten; `stw` returns their final states, slot by slot.
static int32_t pn_solve_wide(tog_handle* h, const tog_pn_options* opts, bool optimal, const std::vector<int>& trajs,
                             std::vector<PNState>& stw) {
  const long long B = h->B, S = (long long)trajs.size();
  if (!h->ops->pn_wide) return fail(TOG_ERR_UNSUPPORTED, "projected Newton needs n + m <= 64 (a lane per variable of a knot)");
  PNWideBuffers W = {};
  W.SM = std::min(h->n + h->pmax, PN_SM_WIDE_MAX);
  W.nb = h->N + 1;
  W.optimal = optimal ? 1 : 0;
  W.atol = opts->active_set_tolerance;
  W.eps = opts->feasibility_tolerance;
  size_t lim = 0;
  int32_t rc = pn_lds_limit(h, &lim);
  if (rc) return rc;
  const size_t lds = pn_lds_bytes_wide(W.SM) + 512;  // (+ the kernels' static LDS: exchange slots, barrier votes; 272 bytes)
  if (lds > lim)
    return fail(TOG_ERR_UNSUPPORTED, "projected Newton's wide kernels need " + std::to_string(lds) +
                                         " bytes of LDS a workgroup; the device offers " + std::to_string(lim));
  const size_t blk = (size_t)S * W.nb * W.SM * W.SM, vec = (size_t)S * W.nb * W.SM;
  const size_t pm = (size_t)(h->pmax > 0 ? h->pmax : 1);
  const size_t nz = (size_t)S * h->N * (h->n + h->m), nx = (size_t)S * h->N * h->n, nc = (size_t)S * h->N * pm;
  const size_t nu = (size_t)S * (h->N - 1) * h->m, nwt = (size_t)S * ((size_t)h->N * h->n + (size_t)(h->N - 1) * h->m);
  size_t need = sizeof(double) * (4 * blk + 5 * vec + 2 * nx + (h->ops->min_time ? nwt : 0)) +
                sizeof(int) * (nc + (size_t)S * h->N + 2 * (size_t)S * W.nb) + sizeof(PNState) * (size_t)S;
  if (optimal) need += sizeof(double) * (2 * blk + 2 * vec + 3 * nz + 4 * nx + 3 * nc + nu) + sizeof(int) * (size_t)S * W.nb;
  size_t fr = 0, tot = 0;
  HIPCHECK(hipMemGetInfo(&fr, &tot));
  if (need > fr)
    return fail(TOG_ERR_NOMEM, "projected Newton wide workspace of " + std::to_string(S) + " trajectories (" +
                                   std::to_string(need >> 20) + " MiB) exceeds free device memory (" + std::to_string(fr >> 20) + " MiB)");
  ScopedDev mem;
  int* d_slot = nullptr;
  hipError_t e = hipSuccess;
  auto get = [&](auto** p, size_t count) {
    if (e == hipSuccess) e = mem.get(p, count);
  };
  get(&W.Sd, blk), get(&W.So, blk), get(&W.Ld, blk), get(&W.Lo, blk);
  get(&W.yv, vec), get(&W.xv, vec), get(&W.rv, vec), get(&W.wv, vec), get(&W.dv, vec);
  get(&W.yd, nx), get(&W.Xs, nx), get(&W.act, nc), get(&W.na, (size_t)S * h->N), get(&W.sz, (size_t)S * W.nb);
  get(&W.st, (size_t)S), get(&d_slot, (size_t)S);
  if (h->ops->min_time) get(&W.wt, nwt);
  if (optimal) {
    get(&W.Ld2, blk), get(&W.Lo2, blk), get(&W.lb, vec), get(&W.tb, vec), get(&W.g, nz), get(&W.rz, nz), get(&W.dz, nz);
    get(&W.nu, nx), get(&W.dnu, nx), get(&W.nut, nx), get(&W.Xv, nx), get(&W.lc, nc), get(&W.dlc, nc), get(&W.lct, nc);
    get(&W.Uv, nu), get(&W.szS, (size_t)S * W.nb);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(TOG_ERR_NOMEM, std::string("projected Newton wide workspace: ") + hipGetErrorString(e));
  }
  W.slot = d_slot;
  std::vector<int> slot_of(B, -1);
  for (long long s = 0; s < S; s++) {
    slot_of[trajs[s]] = (int)s;
    for (int step = 0; step < opts->n_steps; step++)
      h->pn_hist[2 * ((size_t)trajs[s] * opts->n_steps + step)] = h->pn_hist[2 * ((size_t)trajs[s] * opts->n_steps + step) + 1] = NAN;
  }
  // (the stream is idle: the narrow pass ended with a synchronize)
  HIPCHECK(hipMemcpy(d_slot, trajs.data(), sizeof(int) * S, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h->pn_slot_of, slot_of.data(), sizeof(int) * B, hipMemcpyHostToDevice));
  HIPCHECK(hipMemsetAsync(W.st, 0, sizeof(PNState) * S, h->stream));
  if (optimal) {  // PrimalDual(prob): zero duals
    HIPCHECK(hipMemsetAsync(W.nu, 0, sizeof(double) * nx, h->stream));
    HIPCHECK(hipMemsetAsync(W.lc, 0, sizeof(double) * nc, h->stream));
  }
  const long long tx = (long long)h->N * h->n, tu = (long long)(h->N - 1) * h->m;
  hipLaunchKernelGGL(k_pn_wide_gate, dim3((unsigned)B), dim3(64), 0, h->stream, h->buf.st, h->pn_slot_of, h->pn_park,
                     h->buf.X, h->buf.U, h->pn_X0, h->pn_U0, tx, tu, 1);
  rc = pn_pass(h, opts, optimal, W.st, S, stw,
               [&](int phase) { return h->ops->pn_wide(h->dP, h->buf, W, S, h->integ, phase, h->stream); },
               [&](long long s) { return trajs[s]; });
  if (rc) return rc;
  hipLaunchKernelGGL(k_pn_wide_gate, dim3((unsigned)B), dim3(64), 0, h->stream, h->buf.st, h->pn_slot_of, h->pn_park,
                     h->buf.X, h->buf.U, h->pn_X0, h->pn_U0, tx, tu, 0);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(h->stream));  // the workspace is released on return
  return TOG_OK;
}

extern "C" {

int32_t tog_version(void) { return TOG_ABI_VERSION; }
// (internal) the error path of tog_altro.cpp: records the message for tog_last_error
int32_t tog__fail(int32_t code, const char* msg) { return fail(code, msg); }

int32_t tog_model_load(const char* path, tog_model** out) {
  if (!path || !out) return fail(TOG_ERR_ARG, "null argument");
  *out = nullptr;
  void* so = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!so) return fail(TOG_ERR_ARG, std::string("cannot load model plugin: ") + dlerror());
  auto fp = reinterpret_cast<long long (*)()>(dlsym(so, "tog_plugin_fingerprint"));
  auto ops = reinterpret_cast<const ModelOps* (*)()>(dlsym(so, "tog_plugin_ops"));
  auto opi = reinterpret_cast<const ModelOps* (*)()>(dlsym(so, "tog_plugin_ops_infeasible"));
  auto opm = reinterpret_cast<const ModelOps* (*)()>(dlsym(so, "tog_plugin_ops_min_time"));
  if (!fp || !ops || !opi || !opm) {
    dlclose(so);
    return fail(TOG_ERR_ARG, "not a libtog model plugin (TOG_PLUGIN symbols missing)");
  }
  if (fp() != plugin_fingerprint()) {
    dlclose(so);
    return fail(TOG_ERR_ARG, "model plugin was built against different libtog headers");
  }
  tog_model* m = new tog_model{so, ops(), opi(), opm()};
  *out = m;
  return TOG_OK;
}

int32_t tog_model_dims(const tog_model* model, int32_t* n, int32_t* m) {
  if (!model || !n || !m) return fail(TOG_ERR_ARG, "null argument");
  *n = model->ops->n;
  *m = model->ops->m;
  return TOG_OK;
}

int32_t tog_model_free(tog_model* model) {
  if (!model) return fail(TOG_ERR_ARG, "null model");
  dlclose(model->so);
  delete model;
  return TOG_OK;
}

// GenericCost plugins (tog_cost_plugin.hpp): the plugin's kernels evaluate ℓ / ℓf with their
// ForwardDiff-style gradient and Hessian; libtog stages host buffers and checks the results' launch
int32_t tog_generic_cost_load(const char* path, tog_generic_cost** out) {
  if (!path || !out) return fail(TOG_ERR_ARG, "null argument");
  *out = nullptr;
  void* so = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!so) return fail(TOG_ERR_ARG, std::string("cannot load cost plugin: ") + dlerror());
  auto fp = reinterpret_cast<long long (*)()>(dlsym(so, "tog_cost_plugin_fingerprint"));
  auto dims = reinterpret_cast<int (*)(int*, int*)>(dlsym(so, "tog_cost_plugin_dims"));
  auto ex = reinterpret_cast<tog_generic_cost::expand_fn>(dlsym(so, "tog_cost_plugin_expand"));
  if (!fp || !dims || !ex) {
    dlclose(so);
    return fail(TOG_ERR_ARG, "not a libtog cost plugin (TOG_COST_PLUGIN symbols missing)");
  }
  if (fp() != cost_plugin_fingerprint()) {
    dlclose(so);
    return fail(TOG_ERR_ARG, "cost plugin was built against different libtog headers");
  }
  tog_generic_cost* c = new tog_generic_cost{so, 0, 0, ex};
  dims(&c->n, &c->m);
  *out = c;
  return TOG_OK;
}

int32_t tog_generic_cost_dims(const tog_generic_cost* cost, int32_t* n, int32_t* m) {
  if (!cost || !n || !m) return fail(TOG_ERR_ARG, "null argument");
  *n = cost->n;
  *m = cost->m;
  return TOG_OK;
}

int32_t tog_generic_cost_expand_device(const tog_generic_cost* cost, int32_t terminal, const double* X, const double* U,
                               int64_t count, double* J, double* Ex, double* Eu, double* Exx, double* Euu,
                               double* Eux, void* hip_stream) {
  if (!cost) return fail(TOG_ERR_ARG, "null cost");
  if (count < 0) return fail(TOG_ERR_ARG, "count < 0");
  if (count == 0) return TOG_OK;
  if (!X || !J || !Ex || !Exx || (!terminal && (!U || !Eu || !Euu || !Eux)))
    return fail(TOG_ERR_ARG, "null buffer");
  if (cost->ex(terminal ? 1 : 0, X, U, count, J, Ex, Eu, Exx, Euu, Eux, hip_stream) != 0)
    return fail(TOG_ERR_DEVICE, "cost plugin launch failed");
  return TOG_OK;
}

int32_t tog_generic_cost_expand(const tog_generic_cost* cost, int32_t device, int32_t terminal, const double* X, const double* U,
                        int64_t count, double* J, double* Ex, double* Eu, double* Exx, double* Euu, double* Eux) {
  if (!cost) return fail(TOG_ERR_ARG, "null cost");
  if (count < 0) return fail(TOG_ERR_ARG, "count < 0");
  if (count == 0) return TOG_OK;
  if (!X || !J || !Ex || !Exx || (!terminal && (!U || !Eu || !Euu || !Eux)))
    return fail(TOG_ERR_ARG, "null buffer");
  const size_t n = cost->n, m = terminal ? 0 : cost->m, c = (size_t)count;
  // one device block: X | U | J | Ex | Eu | Exx | Euu | Eux
  const size_t sz[8] = {n * c, m * c, c, n * c, m * c, n * n * c, m * m * c, m * n * c};
  size_t tot = 0;
  for (size_t v : sz) tot += v;
  HIPCHECK(hipSetDevice(device));
  double* d = nullptr;
  HIPCHECK(hipMalloc(&d, tot * sizeof(double)));
  double* p[8];
  size_t o = 0;
  for (int i = 0; i < 8; i++) {
    p[i] = d + o;
    o += sz[i];
  }
  hipError_t e = hipMemcpy(p[0], X, sz[0] * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && m) e = hipMemcpy(p[1], U, sz[1] * sizeof(double), hipMemcpyHostToDevice);
  int rc = TOG_OK;
  if (e == hipSuccess) {
    rc = cost->ex(terminal ? 1 : 0, p[0], p[1], count, p[2], p[3], p[4], p[5], p[6], p[7], nullptr);
    if (rc != 0) rc = fail(TOG_ERR_DEVICE, "cost plugin launch failed");
  }
  if (e == hipSuccess && rc == TOG_OK) e = hipDeviceSynchronize();
  double* outs[6] = {J, Ex, Eu, Exx, Euu, Eux};
  for (int i = 0; i < 6 && e == hipSuccess && rc == TOG_OK; i++)
    if (sz[i + 2]) e = hipMemcpy(outs[i], p[i + 2], sz[i + 2] * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(TOG_ERR_DEVICE, std::string("tog_cost_expand: ") + hipGetErrorString(e));
  return rc;
}

int32_t tog_generic_cost_free(tog_generic_cost* cost) {
  if (!cost) return fail(TOG_ERR_ARG, "null cost");
  dlclose(cost->so);
  delete cost;
  return TOG_OK;
}

// dynamics_bias(state) of an RBD model at x = [q; v] (RigidBodyDynamics, used by
// hold_trajectory dynamics/kuka.jl:117-132): host evaluation of the same model code the kernels run.
int tog_dynamics_bias(int32_t model, const double* x, double* tau) {
  if (!x || !tau) return TOG_ERR_ARG;
  if (model != TOG_MODEL_KUKA) return TOG_ERR_UNSUPPORTED;
  double c[7], s[7];
  Kuka::bias<double>(tau, c, s, x, x + 7);
  return TOG_OK;
}

int32_t tog_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

void tog_default_options(tog_options* o) {
  memset(o, 0, sizeof(*o));
  o->cost_tolerance = 1e-4;
  o->gradient_norm_tolerance = 1e-5;
  o->iterations = 300;
  o->dJ_counter_limit = 10;
  o->square_root = 0;
  o->bp_reg_type = 0;
  o->gradient_type = 0;
  o->iterations_linesearch = 20;
  o->line_search_lower_bound = 1e-8;
  o->line_search_upper_bound = 10.0;
  o->bp_reg_increase_factor = 1.6;
  o->bp_reg_max = 1e8;
  o->bp_reg_min = 1e-8;
  o->bp_reg_fp = 10.0;
  o->max_cost_value = 1e8;
  o->max_state_value = 1e8;
  o->max_control_value = 1e8;
  o->al_cost_tolerance = 1e-4;
  o->al_cost_tolerance_intermediate = 1e-3;
  o->al_gradient_norm_tolerance = 1e-5;
  o->al_gradient_norm_tolerance_intermediate = 1e-5;
  o->constraint_tolerance = 1e-3;
  o->dual_min = -1e8;
  o->dual_max = 1e8;
  o->penalty_max = 1e8;
  o->penalty_initial = 1.0;
  o->penalty_scaling = 10.0;
  o->al_iterations = 30;
  o->kickout_max_penalty = 0;
}

const char* tog_last_error(void) { return g_err.c_str(); }


// =============================================================================================
// Multi-device handles (tog_create_multi): the batch is split into
// contiguous slices, one plain handle (device buffers + stream) per device. Trajectories are
// independent (§8(e)), so every step-level and solve-level call is the same call on each slice;
// launches are asynchronous per device, so the devices run concurrently. Host arrays are split
// and gathered along the batch axis, which is the outermost axis of every field.
// =============================================================================================
static bool is_multi(const tog_handle* h) { return h && !h->parts.empty(); }

// doubles per trajectory of a host-side field array (tog_get / tog_set layouts)
static size_t per_traj(const tog_handle* h, int field) {
  const size_t n = h->n, m = h->m, N = h->N, P1 = h->pmax > 0 ? h->pmax : 1;
  switch (field) {
    case TOG_FIELD_X: case TOG_FIELD_XBAR: return N * n;
    case TOG_FIELD_U: case TOG_FIELD_UBAR: case TOG_FIELD_D: return (N - 1) * m;
    case TOG_FIELD_K: return (N - 1) * m * n;
    case TOG_FIELD_A: return (N - 1) * n * n;
    case TOG_FIELD_B: return (N - 1) * n * m;
    case TOG_FIELD_S: return N * n * n;
    case TOG_FIELD_SX: return N * n;
    case TOG_FIELD_DV: case TOG_FIELD_RHO: return 2;
    case TOG_FIELD_LAMBDA: case TOG_FIELD_MU: case TOG_FIELD_C: return N * P1;
    case TOG_FIELD_X0: return n;
    case TOG_FIELD_STATS: return TOG_NSTATS;
    case TOG_FIELD_Q: return N * (size_t)h->nq;
    case TOG_FIELD_HIST_INNER: return 3 * (size_t)h->buf.hcap;
    case TOG_FIELD_HIST_OUTER: return 4 * (size_t)h->buf.ocap;
    case TOG_FIELD_HIST_COUNT: return 2;
  }
  return 0;
}

extern "C++" {
template <class F>
static int32_t each_part(tog_handle* h, F&& fn) {
  for (size_t i = 0; i < h->parts.size(); i++) {
    int32_t rc = fn(h->parts[i], (size_t)h->part_off[i]);
    if (rc) return rc;
  }
  return TOG_OK;
}
}  // extern "C++"

int32_t tog_destroy(tog_handle* h) {
  if (!h) return TOG_OK;
  if (is_multi(h)) {
    for (tog_handle* p : h->parts) tog_destroy(p);
    delete h;
    return TOG_OK;
  }
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  if (h->sp.st2) (void)hipStreamDestroy(h->sp.st2);
  if (h->sp.fork) (void)hipEventDestroy(h->sp.fork);
  if (h->sp.join) (void)hipEventDestroy(h->sp.join);
  for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->stats_ev) (void)hipEventDestroy(h->stats_ev);
  if (h->sync_ev) (void)hipEventDestroy(h->sync_ev);
  if (h->h_stats) (void)hipHostFree(h->h_stats);
  // streamed solves: the pinned staging (the device twins are in allocs) and the events
  if (h->h_ints) (void)hipHostFree(h->h_ints);
  for (tog_handle::Stage* s : {&h->sin_x0, &h->sin_U, &h->sin_X, &h->sin_tab, &h->sout})
    if (s->h) (void)hipHostFree(s->h);
  for (hipEvent_t e : {h->fin_ev, h->refill_ev, h->gather_ev})
    if (e) (void)hipEventDestroy(e);
  delete h;
  return TOG_OK;
}

// tog_create after argument validation, in parts (create_single below runs them in order). Every early return
// (HIPCHECK, allocation, build_rows) leaves the partially built handle to the caller, which destroys it (streams,
// events, allocations).

// the descriptor's constraint sets as per-knot rows (build_rows)
struct HostRows {
  std::vector<ConRow> rows;
  std::vector<int> off, cnt;  // first row and row count of each knot
  // rows with a state gradient per knot (every row type but the control bounds): the knots whose
  // square-root expansion changes Q.xx (expansion records, tog_bwd_team.hpp ne_of)
  std::vector<int> nx;
};

// 1. h->hostP from the descriptor, the rows and the host plan (tog_host_plan.hpp); no device work
static int32_t fill_problem(tog_handle* h, const tog_problem_desc* d, const tog_options* opts, const HostRows& hr,
                            const tog_plan::CostPlan& cp) {
  const int n = h->n, m = h->m;
  DevProblem& P = h->hostP;
  memset(&P, 0, sizeof(P));
  P.n = n;
  P.m = m;
  P.N = h->N;
  P.pmax = h->pmax;
  P.model = d->model;
  P.integ = d->integrator;
  P.nrows = h->nrows;
  P.B = h->B;
  P.dt = d->dt;
  // P's own cost fields hold knot 0's (the shared one without a table)
  memcpy(P.Q, cp.Q(0), sizeof(double) * n * n);
  memcpy(P.R, cp.R(0), sizeof(double) * m * m);
  memcpy(P.H, cp.H(0), sizeof(double) * m * n);
  memcpy(P.q, cp.q(0), sizeof(double) * n);
  memcpy(P.r, cp.r(0), sizeof(double) * m);
  P.c = cp.c(0);
  memcpy(P.Qf, d->Qf, sizeof(double) * n * n);
  memcpy(P.qf, d->qf, sizeof(double) * n);
  P.cf = d->cf;
  memcpy(P.cQf, cp.cQf.data(), sizeof(double) * n * n);
  memcpy(P.cQ, cp.cQ(0), sizeof(double) * n * n);
  memcpy(P.cR, cp.cR(0), sizeof(double) * m * m);
  P.sqrt_ok = cp.sqrt_ok ? 1 : 0;
  P.diag_cost = cp.diag_cost;
  h->buf.cost_diag = P.diag_cost;
  h->sqrt_ok0 = P.sqrt_ok;
  h->diag0 = P.diag_cost;
  if (opts->square_root && !cp.sqrt_ok)
    return fail(TOG_ERR_ARG, "cost Hessians must be PD for the sqrt backward pass (objective.jl:70-94)");
  // packed std AL expansion records: the Q.xx entries a stage row can change (row_grad's state indices)
  {
    std::vector<unsigned int> masks;
    masks.reserve(hr.rows.size());
    for (const ConRow& r : hr.rows) {
      unsigned int sx = 0;
      switch (r.type) {
        case ROW_XMAX: case ROW_XMIN: case ROW_GOAL: case ROW_MT_EQ: sx = 1u << r.idx; break;
        case ROW_UMAX: case ROW_UMIN: case ROW_USLACK: break;
        case ROW_CIRCLE: sx = 3u; break;
        case ROW_SPHERE: sx = 7u; break;
        default: sx = (1u << n) - 1u;  // user rows: dense
      }
      masks.push_back(sx);
    }
    const tog_plan::QPattern qp = tog_plan::plan_qpattern(n, masks.data(), masks.size());
    for (int c = 0; c < n; c++) {
      P.qpat[c] = qp.qpat[c];
      P.qoff[c] = qp.qoff[c];
    }
    P.qpat_n = qp.qpat_n;
    P.qpat_max = qp.qpat_max;
    // (the expansion's pattern loop: every column within QPK pattern rows; TOG_DENSE_RECORDS=1 runs the
    // general loop, for A/B checks)
    P.qpat_on = (P.qpat_max <= QPK && getenv("TOG_DENSE_RECORDS") == nullptr) ? 1 : 0;
  }
  P.kc = nullptr;
  P.kc_stride = cp.kst;
  P.kc_pad = 0;
  {
    std::vector<int> rt(hr.rows.size()), ri(hr.rows.size());
    for (size_t i = 0; i < hr.rows.size(); i++) {
      rt[i] = hr.rows[i].type;
      ri[i] = hr.rows[i].idx;
    }
    h->goal_err =
        tog_traj::terminal_goal_rows(rt.data(), ri.data(), hr.off.data(), hr.cnt.data(), h->N, n, ROW_GOAL, h->goal_idx);
  }
  P.o = *opts;
  P.R_min_time = (d->flags & TOG_PROB_MIN_TIME) ? d->R_min_time : 0.0;
  return TOG_OK;
}

// 2. the device tables hostP points to (a time-varying Objective's cost table, the constraint rows), then hostP
// itself
static int32_t upload_tables(tog_handle* h, const tog_problem_desc* d, const HostRows& hr,
                             const tog_plan::CostPlan& cp) {
  int rc;
  const int N = h->N;
  DevProblem& P = h->hostP;
  if (d->stage_costs) {
    double* dkc = nullptr;
    if ((rc = dalloc(h, &dkc, cp.kc.size()))) return rc;
    HIPCHECK(hipMemcpy(dkc, cp.kc.data(), sizeof(double) * cp.kc.size(), hipMemcpyHostToDevice));
    P.kc = dkc;
  } else {
    h->kc_row = cp.kc;  // (one row: replicated per knot when per-trajectory data is set, traj_apply)
  }
  h->kc0 = P.kc;
  if ((rc = dalloc(h, &h->d_knot_off, N)) || (rc = dalloc(h, &h->d_knot_cnt, N)) ||
      (rc = dalloc(h, &h->d_knot_nx, N)) || (rc = dalloc(h, &h->d_rows, hr.rows.size() + 1)) ||
      (rc = dalloc(h, &h->dP, 1)))
    return rc;
  HIPCHECK(hipMemcpy(h->d_knot_off, hr.off.data(), sizeof(int) * N, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h->d_knot_cnt, hr.cnt.data(), sizeof(int) * N, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(h->d_knot_nx, hr.nx.data(), sizeof(int) * N, hipMemcpyHostToDevice));
  if (!hr.rows.empty())
    HIPCHECK(hipMemcpy(h->d_rows, hr.rows.data(), sizeof(ConRow) * hr.rows.size(), hipMemcpyHostToDevice));
  P.knot_off = h->d_knot_off;
  P.knot_cnt = h->d_knot_cnt;
  P.knot_nx = h->d_knot_nx;
  P.rows = h->d_rows;
  HIPCHECK(hipMemcpy(h->dP, &P, sizeof(P), hipMemcpyHostToDevice));
  return TOG_OK;
}

// 3. the kernel variants of this problem (h->bwd_team and the launch fields of h->buf); returns whether the line
// search is the candidate-copy one
static bool choose_variants(tog_handle* h, const tog_problem_desc* d, const tog_options* opts, const HostRows& hr) {
  const int n = h->n, m = h->m, N = h->N, nrows = (int)hr.rows.size();
  const ModelOps* ops = h->ops;
  DevBuffers& b = h->buf;
  {
    // TOG_BWD=lds forces the one-wave-per-trajectory LDS backward kernel (A/B checks)
    const char* ev = getenv("TOG_BWD");
    const bool force_lds = ev && strcmp(ev, "lds") == 0;
    // (a time-varying Objective runs the team kernels' TV variants, which read knot k's cost from the table)
    h->bwd_team = (!force_lds && !ops->min_time &&
                   team_rows_fit(hr.off.data(), hr.cnt.data(), hr.rows.data(), N, n, m, nrows))
                      ? 1 : 0;
    for (int sq = 0; sq < 2; sq++) {
      b.bwd_stride2[sq] = ops->team_stride(h->pmax, sq);
      b.bwd_shmem2[sq] = (int)bwd_team_shmem(b.bwd_stride2[sq], ops->team_tpw, nrows, N);
      if (b.bwd_shmem2[sq] > 64 * 1024) h->bwd_team = 0;
    }
  }
  // bulk k_ls_spec: a block's LDS copy of the row tables
  b.rows_lds = row_tables_bytes(nrows, N);
  // the tail rollouts staged through LDS, admissible up to SPEC_TAIL_PMAX rows per knot: k_ls_spec_tail2 (three
  // waves) within 64 KB of LDS, else the one-wave k_ls_spec_tail
  b.spec_tail2_shmem = tog_plan::spec_tail2_lds(n, m, h->pmax);
  b.spec_tail_shmem = tog_plan::spec_tail_lds(n, m, h->pmax);
  b.tv = d->stage_costs ? 1 : 0;
  h->tv0 = b.tv;
  b.dense_stage_knots = 0;  // a stage knot with a state row (its square-root expansion changes Q.xx)
  for (int k = 0; k + 1 < N; k++)
    if (hr.nx[k] > 0) b.dense_stage_knots = 1;
  b.nc = opts->iterations_linesearch + 1 < 64 ? opts->iterations_linesearch + 1 : 64;
  if (b.nc < 1) b.nc = 1;
  b.ncp = (b.nc + 7) & ~7;
  b.nknots = N;
  b.tail = 0;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess) cus = 0;
    b.simds = 4 * cus;
  }
  b.ls_pend_ok = getenv("TOG_LS_NOPEND") ? 0 : 1;
  b.ls_first = LS_FIRST;
  // candidate-copy line search when every trial fits the speculative window (TOG_LS=replay: the
  // replaying k_ls_commit path, for A/B checks)
  const char* ev = getenv("TOG_LS");
  const bool replay = ev && strcmp(ev, "replay") == 0;
  return !replay && opts->iterations_linesearch + 1 <= 64;
}

// 4. every per-trajectory device buffer of the handle
static int32_t allocate(tog_handle* h, const tog_problem_desc* d, bool cand_ls) {
  int rc;
  const size_t B = (size_t)h->B, n = (size_t)h->n, m = (size_t)h->m, N = (size_t)h->N;
  const size_t P1 = (size_t)(h->pmax > 0 ? h->pmax : 1);
  const ModelOps* ops = h->ops;
  DevBuffers& b = h->buf;
  if ((rc = dalloc(h, &b.x0, B * n)) || (rc = dalloc(h, &b.X, B * N * n)) || (rc = dalloc(h, &b.U, B * (N - 1) * m)) ||
      (rc = dalloc(h, &b.Xb, B * N * n)) || (rc = dalloc(h, &b.Ub, B * (N - 1) * m)) ||
      (rc = dalloc(h, &b.AB, B * (N - 1) * n * (n + m))) || (rc = dalloc(h, &b.K, B * (N - 1) * m * n)) ||
      (rc = dalloc(h, &b.d, B * (N - 1) * m)) || (rc = dalloc(h, &b.lam, B * N * P1)) ||
      (rc = dalloc(h, &b.mu, B * N * P1)) || (rc = dalloc(h, &b.C, B * N * P1)) ||
      (rc = dalloc(h, &b.Qscr, B * N * h->nq)) || (rc = dalloc(h, &b.st, B)) ||
      (rc = dalloc(h, &h->d_scratch, B)) || (rc = dalloc(h, &h->d_scratch2, B)) ||
      (rc = dalloc(h, &h->d_iscratch, B)) || (rc = dalloc(h, &h->d_stats, 4)) ||
      (rc = dalloc(h, &h->d_act_list, B)) || (rc = dalloc(h, &h->d_act_count, 1)) ||
      (rc = dalloc(h, &b.lsJ, B * 64)) || (rc = dalloc(h, &b.lsok, B * 64)) ||
      (rc = dalloc(h, &b.ls_list, 2 * B)) || (rc = dalloc(h, &b.ls_count, LS_COUNT_SLOTS)))
    return rc;
  b.Sdbg = nullptr;
  b.sdbg = nullptr;
  b.E = nullptr;
  b.ls_done = b.ls_list + B;  // (the second half of ls_list; its offset is the full batch, never a
                              //  compacted launch's slot count)
  b.act_list = nullptr;  // set only in the launch view of a compacted tail step
  b.act_count = nullptr;
  b.hist_in = nullptr;  // tog_history_enable
  b.hist_out = nullptr;
  b.hcap = 0;
  b.ocap = 0;
  if (h->bwd_team) {  // expansion records of the team backward pass (k_expand_team)
    const size_t ne = n + m + m * m + n * n;
    if ((rc = dalloc(h, &b.E, B * N * ne))) return rc;
  }
  b.jws = nullptr;
  // the RBD model's RK3 Jacobian in stage-chain form (tog_kuka_jac.hpp): KJ_WSK doubles per (trajectory, knot).
  // (The allocation keeps the size of the form it replaced, jws_per_lane doubles for each of a knot's n + m
  // partials, which is the larger.)
  if (ops->jws_per_lane > 0 && d->integrator == TOG_RK3) {
    const size_t lanes = B * (N - 1) * (size_t)(ops->n + ops->m - ops->slack);
    if ((rc = dalloc(h, &b.jws, lanes * (size_t)ops->jws_per_lane))) return rc;
  }
  b.cand = nullptr;
  b.ls_fb = nullptr;
  if (cand_ls) {
    if ((rc = dalloc(h, &b.cand, B * (size_t)b.ncp * N * 4 * ((n + m + 3) / 4))) || (rc = dalloc(h, &b.ls_win, B)) ||
        (rc = dalloc(h, &b.ls_Jw, B)) || (rc = dalloc(h, &b.gk, B * N)) || (rc = dalloc(h, &b.ls_fb, B)))
      return rc;
  }
  return TOG_OK;
}

// 5. reference constructor state: X = NaN, U = 0, K = d = 0, λ = 0, μ = opts.penalty_initial,
// ρ = dρ = 0 (ilqr_solver.jl:118-144, augmented_lagrangian_solver.jl:143-169)
static int32_t reset_state(tog_handle* h) {
  const size_t B = (size_t)h->B, n = (size_t)h->n, m = (size_t)h->m, N = (size_t)h->N;
  const size_t P1 = (size_t)(h->pmax > 0 ? h->pmax : 1);
  DevBuffers& b = h->buf;
  fill(h, b.x0, B * n, 0.0);
  fill(h, b.X, B * N * n, NAN);
  fill(h, b.U, B * (N - 1) * m, 0.0);
  fill(h, b.Xb, B * N * n, 0.0);
  fill(h, b.Ub, B * (N - 1) * m, 0.0);
  fill(h, b.AB, B * (N - 1) * n * (n + m), 0.0);
  fill(h, b.K, B * (N - 1) * m * n, 0.0);
  fill(h, b.d, B * (N - 1) * m, 0.0);
  fill(h, b.lam, B * N * P1, 0.0);
  fill(h, b.mu, B * N * P1, h->opts.penalty_initial);  // init_constraint_trajectories
  fill(h, b.C, B * N * P1, 0.0);
  hipLaunchKernelGGL(k_reset_state, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, b.st, (long long)B, h->opts.penalty_initial);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TOG_OK;
}

static int32_t create_single(tog_handle* h, const tog_problem_desc* d, const tog_options* opts,
                             const ModelOps* ops, int32_t device) {
  h->device = device;
  HIPCHECK(hipSetDevice(device));
  HIPCHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->own_stream = true;
  HIPCHECK(hipStreamCreateWithFlags(&h->sp.st2, hipStreamNonBlocking));
  HIPCHECK(hipEventCreateWithFlags(&h->sp.fork, hipEventDisableTiming));
  HIPCHECK(hipEventCreateWithFlags(&h->sp.join, hipEventDisableTiming));
  h->model = d->model;
  h->integ = d->integrator;
  h->n = d->n;
  h->m = d->m;
  h->N = d->N;
  h->B = d->batch;
  h->opts = *opts;
  h->ops = ops;
  const int n = h->n, m = h->m, N = h->N;
  h->nq = n + m + n * n + m * m + m * n;

  HostRows hr;
  int rc = build_rows(d, ops->slack, ops->pcap, ops->has_con, hr.rows, hr.off, hr.cnt, &h->obs_kind, &h->bnd_trimmed);
  if (rc) return rc;
  h->nrows = (int)hr.rows.size();
  h->pmax = 0;
  hr.nx.assign(N, 0);
  for (int k = 0; k < N; k++) {
    h->pmax = hr.cnt[k] > h->pmax ? hr.cnt[k] : h->pmax;
    for (int r = 0; r < hr.cnt[k]; r++) {
      const int t = hr.rows[hr.off[k] + r].type;
      if (t != ROW_UMAX && t != ROW_UMIN) hr.nx[k]++;
    }
  }
  // the stage cost(s): one for every knot, or a time-varying Objective's table (desc->stage_costs, rows
  // [Q; R; H; q; r; c]); the device table adds each knot's square-root factors cQ, cR (DevProblem::kc)
  const tog_plan::CostPlan cp =
      tog_plan::plan_costs(n, m, N, d->dt, d->Q, d->R, d->H, d->q, d->r, d->c, d->stage_costs, d->Qf);
  if ((rc = fill_problem(h, d, opts, hr, cp)) || (rc = upload_tables(h, d, hr, cp))) return rc;
  const bool cand_ls = choose_variants(h, d, opts, hr);
  if ((rc = allocate(h, d, cand_ls))) return rc;
  return reset_state(h);
}

int32_t tog_create(const tog_problem_desc* d, const tog_options* opts, int32_t device, tog_handle** out) {
  if (!d || !opts || !out) return fail(TOG_ERR_ARG, "null argument");
  *out = nullptr;
  if (d->flags & ~(int32_t)(TOG_PROB_INFEASIBLE | TOG_PROB_MIN_TIME)) return fail(TOG_ERR_ARG, "unknown problem flags");
  if (opts->gradient_type < 0 || opts->gradient_type > 3)
    return fail(TOG_ERR_ARG, "gradient_type must be 0 (:todorov), 1 (:feedforward), 2 (:ℓ2) or 3 (:ℓinf)");
  if ((d->flags & TOG_PROB_MIN_TIME) && opts->square_root)
    return fail(TOG_ERR_UNSUPPORTED, "minimum time: MinTimeCost has no square-root expansion (std backward pass)");
  const ModelOps* ops = ops_for(d->model, (d->flags & TOG_PROB_INFEASIBLE) != 0, (d->flags & TOG_PROB_MIN_TIME) != 0,
                                d->user_model, d->integrator);
  if (!ops) return fail(TOG_ERR_UNSUPPORTED, "model not built");
  if (d->n != ops->n || d->m != ops->m) return fail(TOG_ERR_ARG, "n, m do not match the model");
  if (d->N < 2) return fail(TOG_ERR_ARG, "N must be >= 2");
  if (d->batch < 1) return fail(TOG_ERR_ARG, "batch must be >= 1");
  if (!(d->dt > 0)) return fail(TOG_ERR_ARG, "dt must be strictly positive");  // src/problem.jl:66-68
  if (d->integrator != TOG_RK3 && d->integrator != TOG_RK4 && d->integrator != TOG_MIDPOINT &&
      d->integrator != TOG_RK3_IMPLICIT && d->integrator != TOG_MIDPOINT_IMPLICIT)
    return fail(TOG_ERR_UNSUPPORTED, "integrator");
  if ((d->integrator == TOG_RK3_IMPLICIT || d->integrator == TOG_MIDPOINT_IMPLICIT) && !ops->implicit)
    return fail(TOG_ERR_UNSUPPORTED, "implicit integrators are built for models with n <= 4 and the quadrotor (no slack controls)");
  int ndev = tog_device_count();
  if (device < 0 || device >= ndev) return fail(TOG_ERR_DEVICE, "no such HIP device");
  tog_handle* h = new tog_handle();
  const int32_t rc = create_single(h, d, opts, ops, device);
  if (rc) {
    tog_destroy(h);
    return rc;
  }
  *out = h;
  return TOG_OK;
}

int32_t tog_create_multi(const tog_problem_desc* d, const tog_options* opts, const int32_t* devices,
                         int32_t ndev, tog_handle** out) {
  if (!d || !opts || !devices || !out) return fail(TOG_ERR_ARG, "null argument");
  *out = nullptr;
  if (ndev < 1) return fail(TOG_ERR_ARG, "ndev must be >= 1");
  if (d->batch < ndev) return fail(TOG_ERR_ARG, "batch must be >= ndev");
  tog_handle* h = new tog_handle();
  const long long B = d->batch, base = B / ndev, rem = B % ndev;
  long long off = 0;
  for (int i = 0; i < ndev; i++) {
    tog_problem_desc di = *d;
    di.batch = base + (i < rem ? 1 : 0);
    tog_handle* p = nullptr;
    int32_t rc = tog_create(&di, opts, devices[i], &p);
    if (rc) {
      const std::string msg = g_err;
      tog_destroy(h);
      return fail(rc, "device " + std::to_string(devices[i]) + ": " + msg);
    }
    h->parts.push_back(p);
    h->part_off.push_back(off);
    off += di.batch;
  }
  h->part_off.push_back(off);
  tog_handle* p0 = h->parts[0];
  h->device = p0->device;
  h->model = p0->model;
  h->integ = p0->integ;
  h->n = p0->n;
  h->m = p0->m;
  h->N = p0->N;
  h->pmax = p0->pmax;
  h->nq = p0->nq;
  h->B = B;
  h->opts = *opts;
  *out = h;
  return TOG_OK;
}

int32_t tog_set_stream(tog_handle* h, void* s) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return fail(TOG_ERR_UNSUPPORTED, "tog_set_stream: a multi-device handle owns one stream per device");
  HIPCHECK(hipSetDevice(h->device));
  HIPCHECK(hipStreamSynchronize(h->stream));
  if (h->own_stream) HIPCHECK(hipStreamDestroy(h->stream));
  if (s) {
    h->stream = (hipStream_t)s;
    h->own_stream = false;
  } else {
    HIPCHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
  }
  return TOG_OK;
}

int32_t tog_synchronize(tog_handle* h) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [](tog_handle* p, size_t) { return tog_synchronize(p); });
  HIPCHECK(hipSetDevice(h->device));
  if (!h->sync_ev) HIPCHECK(hipEventCreateWithFlags(&h->sync_ev, hipEventDisableTiming));
  HIPCHECK(hipEventRecord(h->sync_ev, h->stream));
  return wait_event(h->sync_ev, "tog_synchronize");
}

int32_t tog_dims(tog_handle* h, int64_t* o) {
  if (!h || !o) return fail(TOG_ERR_ARG, "null argument");
  o[0] = h->n;
  o[1] = h->m;
  o[2] = h->N;
  o[3] = h->B;
  o[4] = h->pmax;
  o[5] = h->mode;
  return TOG_OK;
}

int32_t tog_history_enable(tog_handle* h, int32_t capacity) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (capacity < 0) return fail(TOG_ERR_ARG, "capacity must be >= 0");
  const int ocap = h->opts.al_iterations + 1 > 1 ? h->opts.al_iterations + 1 : 1;
  if (is_multi(h)) {
    int32_t rc = each_part(h, [&](tog_handle* p, size_t) { return tog_history_enable(p, capacity); });
    h->buf.hcap = capacity;
    h->buf.ocap = capacity > 0 ? ocap : 0;
    return rc;
  }
  HIPCHECK(hipSetDevice(h->device));
  HIPCHECK(hipStreamSynchronize(h->stream));
  DevBuffers& b = h->buf;
  if (capacity == 0) {  // off (the buffers stay allocated until the handle is destroyed)
    b.hist_in = nullptr;
    b.hist_out = nullptr;
    b.hcap = b.ocap = 0;
    return TOG_OK;
  }
  if (capacity > h->hist_cap_alloc || ocap > h->hist_ocap_alloc || !h->hist_in_alloc) {
    // grow: both new buffers before the old ones go, so a failed allocation leaves the handle as it was
    int rc = TOG_OK;
    const bool ok = tog_traj::replace_buffer_pair(
        &h->hist_in_alloc, (size_t)h->B * 3 * capacity, &h->hist_out_alloc, (size_t)h->B * 4 * ocap,
        [&](size_t c) {
          double* p = nullptr;
          rc = dalloc(h, &p, c);
          return rc == TOG_OK ? p : nullptr;
        },
        [&](double* p) { dfree(h, p); });
    if (!ok) return rc;
    h->hist_cap_alloc = capacity;
    h->hist_ocap_alloc = ocap;
  }
  b.hist_in = h->hist_in_alloc;  // a smaller capacity reuses the allocation (records are strided by hcap)
  b.hist_out = h->hist_out_alloc;
  b.hcap = capacity;
  b.ocap = ocap;
  return TOG_OK;
}

static size_t field_count(tog_handle* h, int field, double** dptr) {
  const size_t B = h->B, n = h->n, m = h->m, N = h->N, P1 = h->pmax > 0 ? h->pmax : 1;
  DevBuffers& b = h->buf;
  switch (field) {
    case TOG_FIELD_X: *dptr = b.X; return B * N * n;
    case TOG_FIELD_U: *dptr = b.U; return B * (N - 1) * m;
    case TOG_FIELD_XBAR: *dptr = b.Xb; return B * N * n;
    case TOG_FIELD_UBAR: *dptr = b.Ub; return B * (N - 1) * m;
    case TOG_FIELD_K: *dptr = b.K; return B * (N - 1) * m * n;
    case TOG_FIELD_D: *dptr = b.d; return B * (N - 1) * m;
    case TOG_FIELD_LAMBDA: *dptr = b.lam; return B * N * P1;
    case TOG_FIELD_MU: *dptr = b.mu; return B * N * P1;
    case TOG_FIELD_C: *dptr = b.C; return B * N * P1;
    case TOG_FIELD_X0: *dptr = b.x0; return B * n;
    case TOG_FIELD_S: *dptr = b.Sdbg; return B * N * n * n;
    case TOG_FIELD_SX: *dptr = b.sdbg; return B * N * n;
    case TOG_FIELD_Q: *dptr = b.Qscr; return B * N * (size_t)h->nq;
    case TOG_FIELD_HIST_INNER: *dptr = b.hist_in; return B * 3 * (size_t)b.hcap;
    case TOG_FIELD_HIST_OUTER: *dptr = b.hist_out; return B * 4 * (size_t)b.ocap;
  }
  *dptr = nullptr;
  return 0;
}

int32_t tog_get_device_ptr(tog_handle* h, int32_t field, void** dptr) {
  if (!h || !dptr) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) return fail(TOG_ERR_UNSUPPORTED, "device pointers are per device: use the per-device handles");
  double* p = nullptr;
  field_count(h, field, &p);
  if (field == TOG_FIELD_STATS) {
    *dptr = h->buf.st;
    return TOG_OK;
  }
  if (!p) return fail(TOG_ERR_ARG, "field has no device buffer");
  *dptr = p;
  return TOG_OK;
}

static int get_states(tog_handle* h, std::vector<TrajState>& st) {
  st.resize(h->B);
  HIPCHECK(hipMemcpyAsync(st.data(), h->buf.st, sizeof(TrajState) * h->B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TOG_OK;
}
static int put_states(tog_handle* h, const std::vector<TrajState>& st) {
  HIPCHECK(hipMemcpyAsync(h->buf.st, st.data(), sizeof(TrajState) * h->B, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TOG_OK;
}

// a trajectory's TOG_FIELD_STATS row
static void stats_row(const TrajState& s, double* o) {
  for (int j = 0; j < TOG_NSTATS; j++) o[j] = 0.0;
  o[TOG_STAT_J] = s.J;
  o[TOG_STAT_DJ] = s.dJ;
  o[TOG_STAT_GRADIENT] = s.grad;
  o[TOG_STAT_ITERATIONS] = s.iters;
  o[TOG_STAT_ZERO_COUNT] = s.zero_cnt;
  o[TOG_STAT_ALPHA] = s.alpha;
  o[TOG_STAT_Z] = s.z;
  o[TOG_STAT_C_MAX] = s.c_max;
  o[TOG_STAT_AL_ITER] = s.al_iter;
  o[TOG_STAT_TOTAL_STEPS] = s.total_steps;
  o[TOG_STAT_LS_TRIALS] = s.ls_trials;
  o[TOG_STAT_BP_RESTARTS] = s.bp_restarts;
  o[TOG_STAT_FLAGS] = s.flags | (s.active ? TOG_TRAJ_ACTIVE : 0);
  o[TOG_STAT_PENALTY_MAX] = s.mu_max;
}

int32_t tog_get(tog_handle* h, int32_t field, double* out) {
  if (!h || !out) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) {
    const size_t w = per_traj(h, field);
    if (!w) return fail(TOG_ERR_ARG, "unknown field");
    return each_part(h, [&](tog_handle* p, size_t o) { return tog_get(p, field, out + o * w); });
  }
  HIPCHECK(hipSetDevice(h->device));
  const size_t n = h->n, m = h->m, N = h->N, B = h->B;
  DevBuffers& b = h->buf;
  if (field == TOG_FIELD_A || field == TOG_FIELD_B) {
    // strided extraction of ∇F[k].xx / .xu from the [A|B] blocks
    const size_t L = n + m, cols = (field == TOG_FIELD_A) ? n : m, c0 = (field == TOG_FIELD_A) ? 0 : n;
    HIPCHECK(hipMemcpy2DAsync(out, sizeof(double) * n * cols, b.AB + c0 * n, sizeof(double) * n * L,
                              sizeof(double) * n * cols, B * (N - 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return TOG_OK;
  }
  if (field == TOG_FIELD_HIST_COUNT) {
    std::vector<TrajState> st;
    int rc = get_states(h, st);
    if (rc) return rc;
    for (size_t i = 0; i < B; i++) {
      out[2 * i] = st[i].hn_in;
      out[2 * i + 1] = st[i].hn_out;
    }
    return TOG_OK;
  }
  if ((field == TOG_FIELD_HIST_INNER || field == TOG_FIELD_HIST_OUTER) && !b.hist_in)
    return fail(TOG_ERR_ARG, "iteration histories are off (tog_history_enable)");
  if (field == TOG_FIELD_STATS || field == TOG_FIELD_DV || field == TOG_FIELD_RHO) {
    std::vector<TrajState> st;
    int rc = get_states(h, st);
    if (rc) return rc;
    for (size_t i = 0; i < B; i++) {
      const TrajState& s = st[i];
      if (field == TOG_FIELD_DV) {
        out[2 * i] = s.dV0;
        out[2 * i + 1] = s.dV1;
      } else if (field == TOG_FIELD_RHO) {
        out[2 * i] = s.rho;
        out[2 * i + 1] = s.drho;
      } else {
        stats_row(s, out + i * TOG_NSTATS);
      }
    }
    return TOG_OK;
  }
  double* p = nullptr;
  size_t count = field_count(h, field, &p);
  if (!p) return fail(TOG_ERR_ARG, "field not available (S/SX need a backward pass with TOG_BP_STORE_S)");
  HIPCHECK(hipMemcpyAsync(out, p, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TOG_OK;
}

int32_t tog_set(tog_handle* h, int32_t field, const double* in) {
  if (!h || !in) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) {
    const size_t w = per_traj(h, field);
    if (!w) return fail(TOG_ERR_ARG, "unknown field");
    return each_part(h, [&](tog_handle* p, size_t o) { return tog_set(p, field, in + o * w); });
  }
  HIPCHECK(hipSetDevice(h->device));
  if (field == TOG_FIELD_DV || field == TOG_FIELD_RHO) {
    std::vector<TrajState> st;
    int rc = get_states(h, st);
    if (rc) return rc;
    for (size_t i = 0; i < (size_t)h->B; i++) {
      if (field == TOG_FIELD_DV) {
        st[i].dV0 = in[2 * i];
        st[i].dV1 = in[2 * i + 1];
      } else {
        st[i].rho = in[2 * i];
        st[i].drho = in[2 * i + 1];
      }
    }
    return put_states(h, st);
  }
  if (field == TOG_FIELD_A || field == TOG_FIELD_B || field == TOG_FIELD_STATS || field == TOG_FIELD_HIST_INNER ||
      field == TOG_FIELD_HIST_OUTER || field == TOG_FIELD_HIST_COUNT)
    return fail(TOG_ERR_ARG, "field is read-only");
  double* p = nullptr;
  size_t count = field_count(h, field, &p);
  if (!p) return fail(TOG_ERR_ARG, "field not settable");
  HIPCHECK(hipMemcpyAsync(p, in, sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TOG_OK;
}

int32_t tog_set_state(tog_handle* h, const double* x0, const double* U, const double* X) {
  if (!h || !x0 || !U) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) {
    const size_t n = h->n, m = h->m, N = h->N;
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_set_state(p, x0 + o * n, U + o * (N - 1) * m, X ? X + o * N * n : nullptr);
    });
  }
  HIPCHECK(hipSetDevice(h->device));
  h->last_active = -1.0;  // every trajectory is active again
  const size_t n = h->n, m = h->m, N = h->N, B = h->B;
  HIPCHECK(hipMemcpyAsync(h->buf.x0, x0, sizeof(double) * B * n, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(h->buf.U, U, sizeof(double) * B * (N - 1) * m, hipMemcpyHostToDevice, h->stream));
  if (X)
    HIPCHECK(hipMemcpyAsync(h->buf.X, X, sizeof(double) * B * N * n, hipMemcpyHostToDevice, h->stream));
  else
    fill(h, h->buf.X, B * N * n, NAN);
  hipLaunchKernelGGL(k_reset_state, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, h->buf.st, (long long)B,
                     1.0);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(h->stream));
  return TOG_OK;
}

// ------------------------------------------------------------------------------ per-trajectory data
// the handle's DevProblem after a table changed: the per-knot cost table cost_at reads the per-trajectory terms
// beside (the descriptor's, or N - 1 copies of its one stage cost), the table pointers, the kernel variant flag
static int32_t traj_apply(tog_handle* h) {
  DevProblem& P = h->hostP;
  // (the obstacle table needs no per-knot cost table: cost_at returns the shared cost without one, and the
  // backward kernels read no constraint row, so an obstacle-only handle sets variant bit 1 alone)
  // (nor does the bound table: it replaces a row's limit, which the same readers take through traj_row)
  // (the weight table counts as cost data: cost_at looks for it beside the per-knot table, and the backward
  // kernels' per-knot-cost variants are the ones that read their Hessians through cost_at)
  const bool cost = h->d_lin || h->d_term || h->d_goal || h->d_hess, any = cost || h->d_obs || h->d_bnd;
  if (cost && !h->kc0 && !h->d_kc_rep) {
    const std::vector<double> t = tog_traj::replicate_row(h->kc_row, h->N - 1);
    int32_t rc = dalloc(h, &h->d_kc_rep, t.size());
    if (rc) return rc;
    HIPCHECK(hipMemcpy(h->d_kc_rep, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
  }
  P.kc = h->kc0 ? h->kc0 : (cost ? h->d_kc_rep : nullptr);
  P.lin = h->d_lin;
  P.term = h->d_term;
  P.goal = h->d_goal;
  P.goal_ld = h->n;
  P.obs = h->d_obs;
  P.obs_ld = (int)tog_traj::obs_width((int)h->obs_kind.size());
  P.bnd = h->d_bnd;
  P.bnd_ld = (int)h->bnd_trimmed.size();
  P.hess = h->d_hess;
  P.hess_ld = (int)tog_traj::hess_width(h->n, h->m);
  // (the cost's structure flags are the batch's while the table is set, the descriptor's again without it)
  P.sqrt_ok = h->d_hess ? h->hess_sqrt_ok : h->sqrt_ok0;
  P.diag_cost = h->d_hess ? h->hess_diag : h->diag0;
  h->buf.cost_diag = P.diag_cost;
  h->buf.tv = ((h->tv0 || cost) ? 1 : 0) | (any ? 2 : 0);  // (bit 1: the per-trajectory kernel variants)
  HIPCHECK(hipStreamSynchronize(h->stream));
  HIPCHECK(hipMemcpy(h->dP, &P, sizeof(P), hipMemcpyHostToDevice));
  return TOG_OK;
}
// a table slot <- count doubles of src (null: drop the table); the new buffer exists before the old one goes
static int32_t traj_table(tog_handle* h, double** slot, const double* src, size_t count) {
  HIPCHECK(hipStreamSynchronize(h->stream));  // no kernel in flight reads the old table
  if (!src) {
    tog_traj::drop_buffer(slot, [&](double* p) { dfree(h, p); });
    return TOG_OK;
  }
  const bool ok = tog_traj::replace_buffer(
      slot, src, count,
      [&](size_t c) {
        double* p = nullptr;
        return dalloc(h, &p, c) == TOG_OK ? p : nullptr;
      },
      [&](double* dst, const double* from, size_t c) {
        return hipMemcpy(dst, from, sizeof(double) * c, hipMemcpyHostToDevice) == hipSuccess;
      },
      [&](double* p) { dfree(h, p); });
  return ok ? TOG_OK : fail(TOG_ERR_DEVICE, "per-trajectory table: device allocation or copy failed");
}
static int32_t traj_refuse(const tog_handle* h, const char* who) {
  if (h->ops->slack || h->ops->min_time)
    return fail(TOG_ERR_UNSUPPORTED, std::string(who) + ": infeasible-start and minimum-time problems keep the shared "
                                                         "objective and goal (their augmented costs and rows are built "
                                                         "from the descriptor)");
  return TOG_OK;
}

int32_t tog_set_trajectory_costs(tog_handle* h, int32_t per_knot, const double* lin, const double* term) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (per_knot != 0 && per_knot != 1) return fail(TOG_ERR_ARG, "per_knot must be 0 or 1");
  if (is_multi(h)) {
    const size_t wl = tog_traj::lin_width(h->n, h->m, h->N, per_knot), wt = tog_traj::term_width(h->n);
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_set_trajectory_costs(p, per_knot, tog_traj::part_slice(lin, o, wl), tog_traj::part_slice(term, o, wt));
    });
  }
  int32_t rc = traj_refuse(h, "tog_set_trajectory_costs");
  if (rc) return rc;
  HIPCHECK(hipSetDevice(h->device));
  const size_t B = (size_t)h->B;
  rc = traj_table(h, &h->d_lin, lin, B * tog_traj::lin_width(h->n, h->m, h->N, per_knot));
  if (!rc) {
    h->hostP.lin_per_knot = lin ? per_knot : 0;
    rc = traj_table(h, &h->d_term, term, B * tog_traj::term_width(h->n));
  }
  // (also after a failure: the device's DevProblem must never keep a pointer to a table that was replaced)
  const int32_t ra = traj_apply(h);
  return rc ? rc : ra;
}

int32_t tog_set_trajectory_goals(tog_handle* h, const double* xf) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) {
    const size_t ng = h->parts[0]->goal_idx.size();
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_set_trajectory_goals(p, tog_traj::part_slice(xf, o, ng));
    });
  }
  int32_t rc = traj_refuse(h, "tog_set_trajectory_goals");
  if (rc) return rc;
  if (h->goal_idx.empty() && h->goal_err.empty())
    return fail(TOG_ERR_ARG, "tog_set_trajectory_goals: the problem's terminal set has no goal constraint");
  if (!h->goal_err.empty()) return fail(TOG_ERR_UNSUPPORTED, h->goal_err);
  HIPCHECK(hipSetDevice(h->device));
  if (xf) {
    const std::vector<double> t = tog_traj::goal_table(xf, h->goal_idx, h->n, h->B);
    rc = traj_table(h, &h->d_goal, t.data(), t.size());
  } else {
    rc = traj_table(h, &h->d_goal, nullptr, 0);
  }
  const int32_t ra = traj_apply(h);
  return rc ? rc : ra;
}

int32_t tog_set_trajectory_obstacles(tog_handle* h, const double* obs) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) {
    const size_t w = tog_traj::obs_width((int)h->parts[0]->obs_kind.size());
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_set_trajectory_obstacles(p, tog_traj::part_slice(obs, o, w));
    });
  }
  if (h->ops->slack || h->ops->min_time) return fail(TOG_ERR_UNSUPPORTED, tog_traj::obstacles_refuse_text());
  if (h->obs_kind.empty()) return fail(TOG_ERR_ARG, tog_traj::obstacles_none_text());
  HIPCHECK(hipSetDevice(h->device));
  int32_t rc;
  if (obs) {
    const std::vector<double> t = tog_traj::obstacle_table(obs, h->obs_kind, h->B);
    rc = traj_table(h, &h->d_obs, t.data(), t.size());
  } else {
    rc = traj_table(h, &h->d_obs, nullptr, 0);
  }
  const int32_t ra = traj_apply(h);
  return rc ? rc : ra;
}

int32_t tog_set_trajectory_bounds(tog_handle* h, const double* bnd) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) {
    const size_t w = h->parts[0]->bnd_trimmed.size();
    const tog_handle* p0 = h->parts[0];
    // (the whole table is checked before any part takes its slice: a refused table leaves every part's in place)
    if (bnd && !p0->ops->slack && !p0->ops->min_time && w > 0) {
      long long Ball = 0;
      for (const tog_handle* p : h->parts) Ball += p->B;
      const std::string err = tog_traj::bound_table_check(bnd, p0->bnd_trimmed, Ball);
      if (!err.empty()) return fail(TOG_ERR_ARG, err);
    }
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_set_trajectory_bounds(p, tog_traj::part_slice(bnd, o, w));
    });
  }
  if (h->ops->slack || h->ops->min_time) return fail(TOG_ERR_UNSUPPORTED, tog_traj::bounds_refuse_text());
  if (h->bnd_trimmed.empty()) return fail(TOG_ERR_ARG, tog_traj::bounds_none_text());
  if (bnd) {
    const std::string err = tog_traj::bound_table_check(bnd, h->bnd_trimmed, h->B);
    if (!err.empty()) return fail(TOG_ERR_ARG, err);  // (the table in place stays)
  }
  HIPCHECK(hipSetDevice(h->device));
  const int32_t rc = traj_table(h, &h->d_bnd, bnd, bnd ? h->bnd_trimmed.size() * (size_t)h->B : 0);
  const int32_t ra = traj_apply(h);
  return rc ? rc : ra;
}

int32_t tog_set_trajectory_weights(tog_handle* h, const double* W) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) {
    const tog_handle* p0 = h->parts[0];
    const size_t w = tog_traj::weights_width(p0->n, p0->m);
    // (the whole table is checked before any part takes its slice: a refused table leaves every part's in place)
    if (W && !p0->ops->slack && !p0->ops->min_time && !p0->kc0) {
      long long Ball = 0;
      for (const tog_handle* p : h->parts) Ball += p->B;
      std::string err = tog_traj::weight_table_check(W, p0->n, p0->m, Ball);
      if (err.empty() && p0->opts.square_root)
        err = tog_traj::weight_pd_text(tog_traj::weight_plan(W, p0->n, p0->m, p0->hostP.dt, Ball));
      if (!err.empty()) return fail(TOG_ERR_ARG, err);
    }
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_set_trajectory_weights(p, tog_traj::part_slice(W, o, w));
    });
  }
  if (int32_t rr = traj_refuse(h, "tog_set_trajectory_weights")) return rr;
  if (h->kc0) return fail(TOG_ERR_UNSUPPORTED, tog_traj::weights_varying_text());
  tog_traj::WeightPlan wp;
  if (W) {
    std::string err = tog_traj::weight_table_check(W, h->n, h->m, h->B);
    if (err.empty()) {
      wp = tog_traj::weight_plan(W, h->n, h->m, h->hostP.dt, h->B);
      if (h->opts.square_root) err = tog_traj::weight_pd_text(wp);
    }
    if (!err.empty()) return fail(TOG_ERR_ARG, err);  // (the table in place stays)
  }
  HIPCHECK(hipSetDevice(h->device));
  const int32_t rc = traj_table(h, &h->d_hess, W ? wp.image.data() : nullptr, wp.image.size());
  if (!rc && W) {
    h->hess_sqrt_ok = wp.sqrt_ok ? 1 : 0;
    h->hess_diag = wp.diag_cost;
  }
  const int32_t ra = traj_apply(h);
  return rc ? rc : ra;
}

// ------------------------------------------------------------------------------ step level
int32_t tog_rollout_open_loop(tog_handle* h) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [](tog_handle* p, size_t) { return tog_rollout_open_loop(p); });
  HIPCHECK(hipSetDevice(h->device));
  h->ops->rollout_open(h->dP, h->buf, h->B, h->integ, h->stream);
  HIPCHECK(hipGetLastError());
  return TOG_OK;
}

int32_t tog_slack_controls(tog_handle* h) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [](tog_handle* p, size_t) { return tog_slack_controls(p); });
  if (!h->ops->slack) return fail(TOG_ERR_ARG, "slack_controls needs a TOG_PROB_INFEASIBLE handle");
  if (h->ops->min_time)
    return fail(TOG_ERR_ARG, "slack_controls runs on the infeasible problem (infeasible.jl:63-80), before "
                             "minimum_time_problem appends h");
  HIPCHECK(hipSetDevice(h->device));
  h->ops->slack_controls(h->dP, h->buf, h->B, h->integ, h->stream);
  HIPCHECK(hipGetLastError());
  return TOG_OK;
}

int32_t tog_jacobians(tog_handle* h) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [](tog_handle* p, size_t) { return tog_jacobians(p); });
  HIPCHECK(hipSetDevice(h->device));
  h->ops->jacobian(h->dP, h->buf, h->B, h->N, h->integ, h->stream);
  HIPCHECK(hipGetLastError());
  return TOG_OK;
}

int32_t tog_update_constraints(tog_handle* h) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [](tog_handle* p, size_t) { return tog_update_constraints(p); });
  HIPCHECK(hipSetDevice(h->device));
  h->ops->update_constraints(h->dP, h->buf, h->B, h->stream);
  HIPCHECK(hipGetLastError());
  return TOG_OK;
}

int32_t tog_cost(tog_handle* h, int32_t al, double* J_out) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h))
    return each_part(h, [&](tog_handle* p, size_t o) { return tog_cost(p, al, J_out ? J_out + o : nullptr); });
  HIPCHECK(hipSetDevice(h->device));
  h->ops->cost(h->dP, h->buf, h->B, al, 0, h->d_scratch, h->stream);
  HIPCHECK(hipGetLastError());
  if (J_out) {
    HIPCHECK(hipMemcpyAsync(J_out, h->d_scratch, sizeof(double) * h->B, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  return TOG_OK;
}

int32_t tog_cost_expansion(tog_handle* h, int32_t sq, int32_t al) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [&](tog_handle* p, size_t) { return tog_cost_expansion(p, sq, al); });
  HIPCHECK(hipSetDevice(h->device));
  if (h->ops->min_time) return fail(TOG_ERR_UNSUPPORTED, "tog_cost_expansion: minimum-time problems (fused in the backward pass)");
  HIPCHECK(hipMemsetAsync(h->d_iscratch, 0, sizeof(int) * h->B, h->stream));
  h->ops->cost_expansion(h->dP, h->buf, h->B, h->N, sq, al, h->d_iscratch, h->stream);
  HIPCHECK(hipGetLastError());
  std::vector<int> f(h->B);
  HIPCHECK(hipMemcpyAsync(f.data(), h->d_iscratch, sizeof(int) * h->B, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));
  for (int v : f)
    if (v) return fail(TOG_ERR_ARG, "PosDefException: cost Hessian not positive definite (objective.jl:70-86)");
  return TOG_OK;
}

int32_t tog_solve_ilqr(tog_handle* h) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  return tog_solve(h, TOG_MODE_ILQR, 0);
}

int32_t tog_solve_al(tog_handle* h) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  return tog_solve(h, TOG_MODE_AL, 0);
}

// Batch steps a solve to completion may take: the iteration budget (iterations, x al_iterations for AL,
// + 1 for the final check) times the line-search rounds one iteration can spread over when its trials
// are run LS_FIRST per batch step (pending mode, ceil(nc / LS_FIRST) rounds). A pending step does not
// advance a trajectory's iteration counter, so a budget of one iteration per step would stop hard
// trajectories before the device-side counters flag them MAX_ITERS. Steps beyond need are free:
// tog_solve stops as soon as no trajectory is active.
int32_t tog_solve_budget(tog_handle* h, int32_t mode) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  const tog_options& o = h->opts;
  long long it = (long long)(o.iterations > 0 ? o.iterations : 0);
  if (mode == TOG_MODE_AL) it *= (o.al_iterations > 0 ? o.al_iterations : 0);
  const int nc = std::max(1, std::min(o.iterations_linesearch + 1, 64));
  const long long rounds = getenv("TOG_LS_NOPEND") ? 1 : (nc + LS_FIRST - 1) / LS_FIRST;
  const long long s = (it + 1) * rounds;
  return (int32_t)std::min<long long>(s, INT32_MAX);
}

int32_t tog_backward_pass(tog_handle* h, int32_t sq, int32_t al, int32_t flags, double* dV_out) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h))
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_backward_pass(p, sq, al, flags, dV_out ? dV_out + 2 * o : nullptr);
    });
  HIPCHECK(hipSetDevice(h->device));
  if (sq && !h->hostP.sqrt_ok) return fail(TOG_ERR_ARG, "cost Hessians must be PD for the sqrt backward pass");
  if ((flags & TOG_BP_STORE_S) && !h->buf.Sdbg) {
    int rc;
    const size_t B = h->B, n = h->n, N = h->N;
    if ((rc = dalloc(h, &h->buf.Sdbg, B * N * n * n)) || (rc = dalloc(h, &h->buf.sdbg, B * N * n))) return rc;
  }
  if (h->bwd_team) h->ops->expand(h->dP, h->buf, h->B, h->N, h->pmax, sq, al, h->stream);
  h->ops->backward(h->dP, h->buf, h->B, sq, al, flags, h->bwd_team, h->stream);
  HIPCHECK(hipGetLastError());
  if (dV_out) return tog_get(h, TOG_FIELD_DV, dV_out);
  return TOG_OK;
}

int32_t tog_forward_pass(tog_handle* h, int32_t al, const double* J_prev, double* J_out) {
  if (!h || !J_prev) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h))
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_forward_pass(p, al, J_prev + o, J_out ? J_out + o : nullptr);
    });
  HIPCHECK(hipSetDevice(h->device));
  HIPCHECK(hipMemcpyAsync(h->d_scratch, J_prev, sizeof(double) * h->B, hipMemcpyHostToDevice, h->stream));
  h->ops->forward(h->dP, h->buf, h->B, h->integ, al ? TOG_MODE_AL : TOG_MODE_ILQR, 0, h->d_scratch, h->d_scratch2,
                  h->stream, nullptr);
  HIPCHECK(hipGetLastError());
  if (J_out) {
    HIPCHECK(hipMemcpyAsync(J_out, h->d_scratch2, sizeof(double) * h->B, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  return TOG_OK;
}

int32_t tog_rollout(tog_handle* h, double alpha, int32_t* ok_out) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h))
    return each_part(h, [&](tog_handle* p, size_t o) { return tog_rollout(p, alpha, ok_out ? ok_out + o : nullptr); });
  HIPCHECK(hipSetDevice(h->device));
  h->ops->rollout(h->dP, h->buf, h->B, h->integ, alpha, h->d_iscratch, h->stream);
  HIPCHECK(hipGetLastError());
  if (ok_out) {
    HIPCHECK(hipMemcpyAsync(ok_out, h->d_iscratch, sizeof(int) * h->B, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  }
  return TOG_OK;
}

// ------------------------------------------------------------------------------ solve level
int32_t tog_solve_init(tog_handle* h, int32_t mode) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) {
    h->mode = mode;
    return each_part(h, [&](tog_handle* p, size_t) { return tog_solve_init(p, mode); });
  }
  if (mode != TOG_MODE_ILQR && mode != TOG_MODE_AL) return fail(TOG_ERR_ARG, "mode");
  HIPCHECK(hipSetDevice(h->device));
  h->mode = mode;
  h->last_active = -1.0;
  h->stats_pending = false;  // a check left open by a failed solve is abandoned (its readback is never read)
  h->ops->init(h->dP, h->buf, h->B, h->integ, mode, h->stream);
  if (h->d_slot_job)  // every slot holds a trajectory again (tog_finished)
    hipLaunchKernelGGL(k_slot_iota, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream, h->d_slot_job,
                       (long long)h->B);
  HIPCHECK(hipGetLastError());
  return TOG_OK;
}

int32_t tog_solve_step(tog_handle* h, int32_t nsteps) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [&](tog_handle* p, size_t) { return tog_solve_step(p, nsteps); });
  HIPCHECK(hipSetDevice(h->device));
  const int al = (h->mode == TOG_MODE_AL);
  // few trajectories (a small batch, or the convergence tail as of the last host readback of n_active):
  // every trial in one speculative round, so the forward pass is one rollout chain and every step
  // completes an iteration of every active trajectory. Otherwise rounds of LS_FIRST trials, an
  // undecided line search continuing in the next step (pending mode).
  const double few = 65536.0 / h->buf.nc;
  h->buf.ls_first = ((double)h->B <= few || (h->last_active >= 0.0 && h->last_active <= few)) ? h->buf.nc : LS_FIRST;
  // convergence tail (or a small batch): the latency-sized backward kernels (k_bwd_team WPE = 1)
  h->buf.tail = ((double)h->B <= TAIL_ACTIVE || (h->last_active >= 0.0 && h->last_active <= TAIL_ACTIVE)) ? 1 : 0;
  // In the tail the kernels launch over the active trajectories only: k_list_active lists them once per
  // call, and each launch covers ceil(last_active) slots instead of the whole batch (traj_of_slot,
  // tog_kernels.hpp). Within a call trajectories only ever finish, so the list stays a superset of the active
  // set for the call's steps, and every kernel still checks `active`. Between calls a slot may start a new
  // trajectory (tog_refill, the streamed solves): the list is rebuilt by the next call, and the refill keeps
  // last_active an upper bound of the active count (it adds the slots it refills), so the launch width covers
  // the new list. Refills therefore happen between tog_solve_step calls only.
  DevBuffers Bt = h->buf;
  long long Bl = h->B;
  if (h->buf.tail && h->last_active >= 0.0 && h->last_active < (double)h->B && !getenv("TOG_NO_COMPACT")) {
    if (h->last_active == 0.0) return TOG_OK;  // nothing left to step
    Bl = (long long)ceil(h->last_active);
    HIPCHECK(hipMemsetAsync(h->d_act_count, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_list_active, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream, h->buf.st,
                       (long long)h->B, h->d_act_list, h->d_act_count);
    Bt.act_list = h->d_act_list;
    Bt.act_count = h->d_act_count;
  }
  for (int i = 0; i < nsteps; i++) {
    // a tail step's Jacobians and expansion as one launch (k_tail_prepare, timed as the Jacobian: no expansion
    // launch is recorded for such a step), or the two as in the bulk
    int fused = 0;
    timed(h, TOG_KERNEL_JACOBIAN, [&] {
      fused = h->ops->tail_prepare(h->dP, Bt, Bl, h->N, h->pmax, h->integ, h->opts.square_root, al, h->bwd_team,
                                   h->stream);
      if (!fused) h->ops->jacobian(h->dP, Bt, Bl, h->N, h->integ, h->stream);
    });
    if (h->bwd_team && !fused)
      timed(h, TOG_KERNEL_EXPANSION, [&] {
        h->ops->expand(h->dP, Bt, Bl, h->N, h->pmax, h->opts.square_root, al, h->stream);
      });
    timed(h, TOG_KERNEL_BACKWARD,
          [&] { h->ops->backward(h->dP, Bt, Bl, h->opts.square_root, al, 0, h->bwd_team, h->stream); });
    timed(h, TOG_KERNEL_FORWARD,
          [&] { h->ops->forward(h->dP, Bt, Bl, h->integ, h->mode, 1, nullptr, nullptr, h->stream, &h->sp); });
  }
  HIPCHECK(hipGetLastError());
  return TOG_OK;
}

int32_t tog_batch_stats_device(tog_handle* h, void* dptr3) {
  if (!h || !dptr3) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) return fail(TOG_ERR_UNSUPPORTED, "device pointers are per device: use tog_batch_stats");
  HIPCHECK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_batch_stats, dim3(1), dim3(1024), 0, h->stream, h->buf.st, (long long)h->B, (double*)dptr3);
  HIPCHECK(hipGetLastError());
  return TOG_OK;
}

int32_t tog_batch_stats(tog_handle* h, double* out3) {
  if (!h || !out3) return fail(TOG_ERR_ARG, "null argument");
  // (a multi-device handle queues every device's reduction before it gathers: _begin / _end fan out)
  int32_t rc = tog_batch_stats_begin(h);
  return rc ? rc : tog_batch_stats_end(h, out3);
}

int32_t tog_batch_stats_begin(tog_handle* h) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [](tog_handle* p, size_t) { return tog_batch_stats_begin(p); });
  HIPCHECK(hipSetDevice(h->device));
  if (h->stats_pending) return fail(TOG_ERR_ARG, "tog_batch_stats_begin: the previous check was not ended");
  if (!h->h_stats) HIPCHECK(hipHostMalloc((void**)&h->h_stats, sizeof(double) * 4, hipHostMallocDefault));
  if (!h->stats_ev) HIPCHECK(hipEventCreateWithFlags(&h->stats_ev, hipEventDisableTiming));
  int rc = tog_batch_stats_device(h, h->d_stats);
  if (rc) return rc;
  HIPCHECK(hipMemcpyAsync(h->h_stats, h->d_stats, sizeof(double) * 3, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipEventRecord(h->stats_ev, h->stream));
  h->stats_pending = true;
  return TOG_OK;
}

int32_t tog_batch_stats_end(tog_handle* h, double* out3) {
  if (!h || !out3) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (tog_handle* p : h->parts) {
      double v[3];
      int32_t rc = tog_batch_stats_end(p, v);
      if (rc) return rc;
      acc[0] += v[0];
      acc[1] += v[1];
      acc[2] = tog_jlmax(acc[2], v[2]);
    }
    out3[0] = acc[0], out3[1] = acc[1], out3[2] = acc[2];
    return TOG_OK;
  }
  if (!h->stats_pending) return fail(TOG_ERR_ARG, "tog_batch_stats_end without tog_batch_stats_begin");
  HIPCHECK(hipSetDevice(h->device));
  h->stats_pending = false;
  const int rc = wait_event(h->stats_ev, "tog_batch_stats");
  if (rc) return rc;
  out3[0] = h->h_stats[0], out3[1] = h->h_stats[1], out3[2] = h->h_stats[2];
  h->last_active = out3[0];
  return TOG_OK;
}

int32_t tog_total_steps(tog_handle* h, int64_t* out) {
  if (!h || !out) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) {
    int64_t t = 0;
    int32_t rc = each_part(h, [&](tog_handle* p, size_t) {
      int64_t v = 0;
      int32_t r = tog_total_steps(p, &v);
      t += v;
      return r;
    });
    *out = t;
    return rc;
  }
  std::vector<TrajState> st;
  int rc = get_states(h, st);
  if (rc) return rc;
  int64_t t = 0;
  for (const auto& s : st) t += s.total_steps;
  *out = t;
  return TOG_OK;
}

// The stopping check is pipelined: chunk i+1's steps are enqueued before the host waits for chunk i's
// statistics, so the device never idles on the host round trip. The last chunk after the batch finished
// runs on inactive trajectories only (every kernel returns at once for them); the arithmetic of the
// solve does not depend on when the host learns the active count (it only picks launch widths).
// after a failure between tog_batch_stats_begin and _end: no check stays pending on any part, so that the
// handle's next tog_batch_stats / tog_solve does not fail with "the previous check was not ended"
static void abandon_stats(tog_handle* h) {
  h->stats_pending = false;
  for (tog_handle* p : h->parts) abandon_stats(p);
}

int32_t tog_solve(tog_handle* h, int32_t mode, int32_t max_steps) {
  int rc = tog_solve_init(h, mode);
  if (rc) return rc;
  if (max_steps <= 0) max_steps = tog_solve_budget(h, mode);
  const int chunk = 4;
  double stats[3];
  int done = chunk < max_steps ? chunk : max_steps;
  if ((rc = tog_solve_step(h, done)) || (rc = tog_batch_stats_begin(h))) return abandon_stats(h), rc;
  while (true) {
    const int next = chunk < max_steps - done ? chunk : max_steps - done;
    if (next > 0 && (rc = tog_solve_step(h, next))) return abandon_stats(h), rc;
    done += next;
    if ((rc = tog_batch_stats_end(h, stats))) return rc;  // the chunk before `next`
    if (stats[0] == 0.0 || next == 0) break;
    if ((rc = tog_batch_stats_begin(h))) return rc;
  }
  return TOG_OK;
}

// ------------------------------------------------------------------------------ streamed solves
// J jobs through the handle's B slots (tog_stream.hpp has the scheduling): k_list_finished lists the slots whose
// trajectory ended, k_gather_slots packs their results for one device -> host copy, k_refill starts the next
// jobs in them. The pieces are exported (tog_finished, tog_get_slots, tog_refill, tog_refill_tables);
// tog_solve_stream is the driver over them.
extern "C++" {
static int32_t stream_refuse(const tog_handle* h, const char* who) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h))
    return fail(TOG_ERR_UNSUPPORTED, std::string(who) + ": not built for tog_create_multi handles (stream one handle per device)");
  return TOG_OK;
}

// while the obstacle table is set: the refill staging carries no obstacle rows, so a refilled slot would keep the
// last job's obstacles (streaming obstacle sweeps is not built)
static int32_t obs_refuse(const tog_handle* h, const char* who) {
  if (h && !is_multi(h) && h->d_obs) return fail(TOG_ERR_UNSUPPORTED, tog_traj::obstacles_set_text(who));
  // likewise the bound table: a refilled slot would keep the last job's limits
  if (h && !is_multi(h) && h->d_bnd) return fail(TOG_ERR_UNSUPPORTED, tog_traj::bounds_set_text(who));
  // and the weight table: a refilled slot would keep the last job's Hessians
  if (h && !is_multi(h) && h->d_hess) return fail(TOG_ERR_UNSUPPORTED, tog_traj::weights_set_text(who));
  return TOG_OK;
}

// first use: the slot arrays, their pinned images and the events
static int32_t stream_alloc(tog_handle* h) {
  if (h->d_slot_job) return TOG_OK;
  const size_t B = (size_t)h->B;
  int rc;
  int* sj = nullptr;
  if ((rc = dalloc(h, &sj, B)) || (rc = dalloc(h, &h->d_fin, B + 1)) || (rc = dalloc(h, &h->d_gl, B)) ||
      (rc = dalloc(h, &h->d_rl, B)) || (rc = dalloc(h, &h->d_rjob, B)))
    return rc;
  HIPCHECK(hipHostMalloc((void**)&h->h_ints, sizeof(int) * (4 * B + 1), hipHostMallocDefault));
  HIPCHECK(hipEventCreateWithFlags(&h->fin_ev, hipEventDisableTiming));
  HIPCHECK(hipEventCreateWithFlags(&h->refill_ev, hipEventDisableTiming));
  HIPCHECK(hipEventCreateWithFlags(&h->gather_ev, hipEventDisableTiming));
  // (as after tog_solve_init: every slot holds its trajectory)
  hipLaunchKernelGGL(k_slot_iota, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, sj, (long long)B);
  HIPCHECK(hipGetLastError());
  h->d_slot_job = sj;
  return TOG_OK;
}
static int* pin_fin(tog_handle* h) { return h->h_ints; }
static int* pin_gl(tog_handle* h) { return h->h_ints + (size_t)h->B + 1; }
static int* pin_rl(tog_handle* h) { return h->h_ints + 2 * (size_t)h->B + 1; }
static int* pin_rjob(tog_handle* h) { return h->h_ints + 3 * (size_t)h->B + 1; }

// a staging pair of at least `count` doubles (sized for B slots of `per_slot` on first use). Growing waits for
// the stream, so nothing in flight reads the old buffers.
static int32_t stage_ensure(tog_handle* h, tog_handle::Stage& s, size_t per_slot, size_t count) {
  if (count <= s.cap && s.h) return TOG_OK;
  const size_t want = std::max(count, per_slot * (size_t)h->B);
  HIPCHECK(hipStreamSynchronize(h->stream));
  if (s.h) (void)hipHostFree(s.h);
  dfree(h, s.d);
  s.h = s.d = nullptr;
  s.cap = 0;
  HIPCHECK(hipHostMalloc((void**)&s.h, sizeof(double) * (want ? want : 1), hipHostMallocDefault));
  const int rc = dalloc(h, &s.d, want);
  if (rc) return rc;
  s.cap = want;
  return TOG_OK;
}

static int32_t check_slots(const tog_handle* h, int32_t count, const int32_t* slots, bool unique, const char* who) {
  if (count < 0 || count > h->B) return fail(TOG_ERR_ARG, std::string(who) + ": count must be in [0, B]");
  if (count > 0 && !slots) return fail(TOG_ERR_ARG, std::string(who) + ": null slot list");
  std::vector<char> seen(unique ? (size_t)h->B : 0, 0);
  for (int i = 0; i < count; i++) {
    if (slots[i] < 0 || slots[i] >= h->B) return fail(TOG_ERR_ARG, std::string(who) + ": slot " + std::to_string(slots[i]) + " out of range");
    if (unique) {
      if (seen[(size_t)slots[i]]) return fail(TOG_ERR_ARG, std::string(who) + ": slot " + std::to_string(slots[i]) + " listed twice");
      seen[(size_t)slots[i]] = 1;
    }
  }
  return TOG_OK;
}

// enqueue: the blocks of `src` (w doubles a slot) of the device list `dlist` into dst
static void gather_enqueue(tog_handle* h, const double* src, size_t w, const int* dlist, int count, double* dst) {
  if (count > 0 && w > 0)
    hipLaunchKernelGGL(k_gather_slots, dim3((unsigned)count), dim3(256), 0, h->stream, src, w, dlist, (long long)h->B, dst);
}
constexpr size_t ST_W = sizeof(TrajState) / sizeof(double);  // a TrajState gathered as doubles
static_assert(sizeof(TrajState) % sizeof(double) == 0, "TrajState is gathered as whole doubles");

// The refill of `count` slots, enqueued (no wait). Job i's data is row src(i) of the arrays (x0 (n, .),
// U (m, N-1, .), X (n, N, .) or null, and the table rows lin, term, xf, each null or (width, .)); job_id(i) is
// what the slot holds from then on. The caller has checked the slots; tables given are tables the handle has.
template <class Src, class Job>
static int32_t refill_enqueue(tog_handle* h, int count, const int* slots, Src&& src, Job&& job_id, const double* x0,
                              const double* U, const double* X, const double* lin, const double* term,
                              const double* xf) {
  if (count <= 0) return TOG_OK;
  int32_t rc;
  const size_t n = h->n, m = h->m, N = h->N, c = (size_t)count;
  const size_t wu = (N - 1) * m, wx = N * n;
  const size_t wl = lin ? tog_traj::lin_width(h->n, h->m, h->N, h->hostP.lin_per_knot) : 0;
  const size_t wt = term ? tog_traj::term_width(h->n) : 0, wg = xf ? n : 0, ng = h->goal_idx.size();
  if (!x0) U = X = nullptr;  // (the tables only)
  if ((x0 && ((rc = stage_ensure(h, h->sin_x0, n, c * n)) || (rc = stage_ensure(h, h->sin_U, wu, c * wu)))) ||
      (X && (rc = stage_ensure(h, h->sin_X, wx, c * wx))) ||
      ((wl + wt + wg) && (rc = stage_ensure(h, h->sin_tab, wl + wt + wg, c * (wl + wt + wg)))))
    return rc;
  if (h->refill_pending) {  // the previous refill's copies have left the pinned buffers
    if ((rc = wait_event(h->refill_ev, "tog_refill"))) return rc;
    h->refill_pending = false;
  }
  int *hl = pin_rl(h), *hj = pin_rjob(h);
  double *tl = h->sin_tab.h, *tt = tl + c * wl, *tg = tt + c * wt;
  for (size_t i = 0; i < c; i++) {
    const size_t j = (size_t)src((int)i);
    hl[i] = slots[i];
    hj[i] = (int)(job_id((int)i) & 0x7fffffffLL);
    if (x0) {
      memcpy(h->sin_x0.h + i * n, x0 + j * n, sizeof(double) * n);
      memcpy(h->sin_U.h + i * wu, U + j * wu, sizeof(double) * wu);
    }
    if (X) memcpy(h->sin_X.h + i * wx, X + j * wx, sizeof(double) * wx);
    if (lin) memcpy(tl + i * wl, lin + j * wl, sizeof(double) * wl);
    if (term) memcpy(tt + i * wt, term + j * wt, sizeof(double) * wt);
    if (xf) {  // the (ng, .) goal values as the device table's (n, .) rows (tog_traj::goal_table)
      const std::vector<double> g = tog_traj::goal_table(xf + j * ng, h->goal_idx, h->n, 1);
      memcpy(tg + i * n, g.data(), sizeof(double) * n);
    }
  }
  hipStream_t st = h->stream;
  HIPCHECK(hipMemcpyAsync(h->d_rl, hl, sizeof(int) * c, hipMemcpyHostToDevice, st));
  HIPCHECK(hipMemcpyAsync(h->d_rjob, hj, sizeof(int) * c, hipMemcpyHostToDevice, st));
  if (x0) {
    HIPCHECK(hipMemcpyAsync(h->sin_x0.d, h->sin_x0.h, sizeof(double) * c * n, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(h->sin_U.d, h->sin_U.h, sizeof(double) * c * wu, hipMemcpyHostToDevice, st));
  }
  if (X) HIPCHECK(hipMemcpyAsync(h->sin_X.d, h->sin_X.h, sizeof(double) * c * wx, hipMemcpyHostToDevice, st));
  if (wl + wt + wg) {
    HIPCHECK(hipMemcpyAsync(h->sin_tab.d, h->sin_tab.h, sizeof(double) * c * (wl + wt + wg), hipMemcpyHostToDevice, st));
    const long long B = h->B;
    double *dl = h->sin_tab.d, *dt = dl + c * wl, *dg = dt + c * wt;
    if (lin) hipLaunchKernelGGL(k_scatter_slots, dim3((unsigned)c), dim3(256), 0, st, h->d_lin, wl, h->d_rl, B, dl);
    if (term) hipLaunchKernelGGL(k_scatter_slots, dim3((unsigned)c), dim3(256), 0, st, h->d_term, wt, h->d_rl, B, dt);
    if (xf) hipLaunchKernelGGL(k_scatter_slots, dim3((unsigned)c), dim3(256), 0, st, h->d_goal, wg, h->d_rl, B, dg);
  }
  if (x0) {
    h->ops->refill(h->dP, h->buf, count, h->N, h->integ, h->mode, h->d_rl, h->sin_x0.d, h->sin_U.d,
                   X ? h->sin_X.d : nullptr, st);
    hipLaunchKernelGGL(k_slots_mark, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, st, h->d_slot_job, h->d_rl,
                       h->d_rjob, count, (long long)h->B);
    // rule 1 (tog_stream.hpp): last_active stays an upper bound of the active count
    if (h->last_active >= 0.0) h->last_active = std::min((double)h->B, h->last_active + (double)count);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(h->refill_ev, st));
  h->refill_pending = true;
  return TOG_OK;
}

// which of the per-trajectory tables a refill may write: only the ones the handle has (its kernel variants
// were chosen when they were set)
static int32_t tables_check(const tog_handle* h, const double* lin, const double* term, const double* xf, const char* who) {
  if ((lin && !h->d_lin) || (term && !h->d_term) || (xf && !h->d_goal))
    return fail(TOG_ERR_UNSUPPORTED, std::string(who) + ": the handle has no such per-trajectory table (set it with "
                                                        "tog_set_trajectory_costs / tog_set_trajectory_goals first)");
  return TOG_OK;
}

// the device of tog_stream::run over one handle
struct StreamDev {
  tog_handle* h;
  const double *x0, *U0, *lin, *term, *xf;
  double *X_out, *U_out, *stats_out;
  std::vector<tog_stream::SlotJob> held;  // the gather in flight
  std::vector<int> sl;
  size_t wx() const { return (size_t)h->N * h->n; }
  size_t wu() const { return (size_t)(h->N - 1) * h->m; }

  int refill(const std::vector<tog_stream::SlotJob>& r) {
    sl.resize(r.size());
    for (size_t i = 0; i < r.size(); i++) sl[i] = r[i].slot;
    return refill_enqueue(
        h, (int)r.size(), sl.data(), [&](int i) { return r[(size_t)i].job; }, [&](int i) { return r[(size_t)i].job; },
        x0, U0, nullptr, lin, term, xf);
  }
  int step(int nsteps, double hint) {
    h->last_active = hint;
    return tog_solve_step(h, nsteps);
  }
  int begin_readback() {
    HIPCHECK(hipMemsetAsync(h->d_fin, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_list_finished, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream, h->buf.st,
                       h->d_slot_job, (long long)h->B, h->d_fin);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(pin_fin(h), h->d_fin, sizeof(int) * ((size_t)h->B + 1), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipEventRecord(h->fin_ev, h->stream));
    return TOG_OK;
  }
  int end_readback(std::vector<int>& list) {
    const int rc = wait_event(h->fin_ev, "tog_solve_stream");
    if (rc) return rc;
    const int* p = pin_fin(h);
    if (p[0] < 0 || p[0] > h->B) return fail(TOG_ERR_DEVICE, "tog_solve_stream: the finished list's count is out of range");
    list.assign(p + 1, p + 1 + p[0]);
    std::sort(list.begin(), list.end());  // (the device list's order depends on the blocks' timing)
    return TOG_OK;
  }
  // the results of the gather in flight, out of the pinned buffer, under their jobs
  int land() {
    if (held.empty()) return TOG_OK;
    const int rc = wait_event(h->gather_ev, "tog_solve_stream");
    if (rc) return rc;
    const size_t c = held.size();
    const double *gx = h->sout.h, *gu = gx + c * wx(), *gs = gu + c * wu();
    for (size_t i = 0; i < c; i++) {
      const size_t j = (size_t)held[i].job;
      if (X_out) memcpy(X_out + j * wx(), gx + i * wx(), sizeof(double) * wx());
      if (U_out) memcpy(U_out + j * wu(), gu + i * wu(), sizeof(double) * wu());
      if (stats_out) {
        TrajState s;
        memcpy(&s, gs + i * ST_W, sizeof(s));
        stats_row(s, stats_out + j * TOG_NSTATS);
      }
    }
    held.clear();
    return TOG_OK;
  }
  int gather(const std::vector<tog_stream::SlotJob>& g, bool) {
    int rc = land();  // (one pinned buffer: the previous gather leaves it first; it completed before this readback)
    if (rc) return rc;
    const size_t c = g.size(), per = wx() + wu() + ST_W;
    if ((rc = stage_ensure(h, h->sout, per, c * per))) return rc;
    int* hl = pin_gl(h);
    for (size_t i = 0; i < c; i++) hl[i] = g[i].slot;
    HIPCHECK(hipMemcpyAsync(h->d_gl, hl, sizeof(int) * c, hipMemcpyHostToDevice, h->stream));
    double *gx = h->sout.d, *gu = gx + c * wx(), *gs = gu + c * wu();
    gather_enqueue(h, h->buf.X, wx(), h->d_gl, (int)c, gx);
    gather_enqueue(h, h->buf.U, wu(), h->d_gl, (int)c, gu);
    gather_enqueue(h, reinterpret_cast<const double*>(h->buf.st), ST_W, h->d_gl, (int)c, gs);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(h->sout.h, h->sout.d, sizeof(double) * c * per, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipEventRecord(h->gather_ev, h->stream));
    held = g;
    return TOG_OK;
  }
  int flush() { return land(); }
};

static int32_t solve_stream(tog_handle* h, int32_t mode, int64_t njobs, const double* x0, const double* U0,
                            const double* lin, const double* term, const double* xf, double* X_out, double* U_out,
                            double* stats_out, int32_t max_steps, int64_t* jobs_done, const char* who) {
  int32_t rc = stream_refuse(h, who);
  if (rc) return rc;
  if (jobs_done) *jobs_done = 0;
  if (mode != TOG_MODE_ILQR && mode != TOG_MODE_AL)
    return fail(TOG_ERR_UNSUPPORTED, std::string(who) + ": streams run TOG_MODE_ILQR and TOG_MODE_AL solves (projected "
                                                        "Newton and the ALTRO flows are not streamed)");
  if (njobs < 0) return fail(TOG_ERR_ARG, std::string(who) + ": njobs < 0");
  if (njobs > 0 && (!x0 || !U0)) return fail(TOG_ERR_ARG, std::string(who) + ": null x0 or U0");
  HIPCHECK(hipSetDevice(h->device));
  if ((rc = stream_alloc(h))) return rc;
  h->mode = mode;
  h->stats_pending = false;
  // every slot empty and inactive; the planner's first refill starts the first min(J, B) jobs
  hipLaunchKernelGGL(k_slots_clear, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream, h->buf.st,
                     h->d_slot_job, (long long)h->B);
  HIPCHECK(hipGetLastError());
  h->last_active = 0.0;
  tog_stream::Planner plan((long long)njobs, (int)h->B);
  StreamDev dev{h, x0, U0, lin, term, xf, X_out, U_out, stats_out, {}, {}};
  const int r = tog_stream::run(plan, dev, 4, max_steps > 0 ? (long long)max_steps : 0);
  if (r == -1 && !plan.error().empty()) return fail(TOG_ERR_DEVICE, std::string(who) + ": " + plan.error());
  if (r) return r;
  if (stats_out)  // jobs never started: zero rows
    for (long long j = plan.started(); j < (long long)njobs; j++)
      memset(stats_out + (size_t)j * TOG_NSTATS, 0, sizeof(double) * TOG_NSTATS);
  if (jobs_done) *jobs_done = plan.finished();
  h->last_active = -1.0;  // (no readback of the batch's active count backs a hint after the stream)
  return TOG_OK;
}
}  // extern "C++"

int32_t tog_finished(tog_handle* h, int32_t* slots_out, int32_t* count_out) {
  int32_t rc = stream_refuse(h, "tog_finished");
  if (rc) return rc;
  if (!slots_out || !count_out) return fail(TOG_ERR_ARG, "null argument");
  HIPCHECK(hipSetDevice(h->device));
  if ((rc = stream_alloc(h))) return rc;
  HIPCHECK(hipMemsetAsync(h->d_fin, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(k_list_finished, dim3((unsigned)((h->B + 255) / 256)), dim3(256), 0, h->stream, h->buf.st,
                     h->d_slot_job, (long long)h->B, h->d_fin);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(pin_fin(h), h->d_fin, sizeof(int) * ((size_t)h->B + 1), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipEventRecord(h->fin_ev, h->stream));
  if ((rc = wait_event(h->fin_ev, "tog_finished"))) return rc;
  const int* p = pin_fin(h);
  if (p[0] < 0 || p[0] > h->B) return fail(TOG_ERR_DEVICE, "tog_finished: the list's count is out of range");
  std::vector<int> l(p + 1, p + 1 + p[0]);
  std::sort(l.begin(), l.end());
  for (size_t i = 0; i < l.size(); i++) slots_out[i] = l[i];
  *count_out = (int32_t)l.size();
  return TOG_OK;
}

int32_t tog_get_slots(tog_handle* h, int32_t field, int32_t count, const int32_t* slots, double* out) {
  int32_t rc = stream_refuse(h, "tog_get_slots");
  if (rc) return rc;
  if ((rc = check_slots(h, count, slots, false, "tog_get_slots"))) return rc;
  if (count == 0) return TOG_OK;
  if (!out) return fail(TOG_ERR_ARG, "null argument");
  HIPCHECK(hipSetDevice(h->device));
  if ((rc = stream_alloc(h))) return rc;
  const bool from_state = field == TOG_FIELD_STATS || field == TOG_FIELD_DV || field == TOG_FIELD_RHO ||
                          field == TOG_FIELD_HIST_COUNT;
  if ((field == TOG_FIELD_HIST_INNER || field == TOG_FIELD_HIST_OUTER) && !h->buf.hist_in)
    return fail(TOG_ERR_ARG, "iteration histories are off (tog_history_enable)");
  double* p = nullptr;
  if (!from_state) field_count(h, field, &p);
  const size_t wo = per_traj(h, field), w = from_state ? ST_W : wo, c = (size_t)count;
  if (!wo || (!from_state && !p))
    return fail(TOG_ERR_ARG, "tog_get_slots: field not available per slot (A, B are strided; S, SX need TOG_BP_STORE_S)");
  if ((rc = stage_ensure(h, h->sout, w, c * w))) return rc;
  HIPCHECK(hipStreamSynchronize(h->stream));  // (the pinned list and buffer are this call's alone)
  int* hl = pin_gl(h);
  for (size_t i = 0; i < c; i++) hl[i] = slots[i];
  HIPCHECK(hipMemcpyAsync(h->d_gl, hl, sizeof(int) * c, hipMemcpyHostToDevice, h->stream));
  gather_enqueue(h, from_state ? reinterpret_cast<const double*>(h->buf.st) : p, w, h->d_gl, count, h->sout.d);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(h->sout.h, h->sout.d, sizeof(double) * c * w, hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipEventRecord(h->gather_ev, h->stream));
  if ((rc = wait_event(h->gather_ev, "tog_get_slots"))) return rc;
  if (!from_state) {
    memcpy(out, h->sout.h, sizeof(double) * c * w);
    return TOG_OK;
  }
  for (size_t i = 0; i < c; i++) {
    TrajState s;
    memcpy(&s, h->sout.h + i * ST_W, sizeof(s));
    double* o = out + i * wo;
    if (field == TOG_FIELD_STATS) {
      stats_row(s, o);
    } else if (field == TOG_FIELD_DV) {
      o[0] = s.dV0, o[1] = s.dV1;
    } else if (field == TOG_FIELD_RHO) {
      o[0] = s.rho, o[1] = s.drho;
    } else {
      o[0] = s.hn_in, o[1] = s.hn_out;
    }
  }
  return TOG_OK;
}

int32_t tog_refill(tog_handle* h, int32_t count, const int32_t* slots, const double* x0, const double* U, const double* X) {
  int32_t rc = stream_refuse(h, "tog_refill");
  if (rc || (rc = obs_refuse(h, "tog_refill"))) return rc;
  if ((rc = check_slots(h, count, slots, true, "tog_refill"))) return rc;
  if (count == 0) return TOG_OK;
  if (!x0 || !U) return fail(TOG_ERR_ARG, "null argument");
  if (h->stats_pending) return fail(TOG_ERR_ARG, "tog_refill: end the pending tog_batch_stats_begin first (its count would miss the refill)");
  HIPCHECK(hipSetDevice(h->device));
  if ((rc = stream_alloc(h))) return rc;
  // no listed slot may still be iterating: their states, gathered
  std::vector<double> st((size_t)count * TOG_NSTATS);
  if ((rc = tog_get_slots(h, TOG_FIELD_STATS, count, slots, st.data()))) return rc;
  for (int i = 0; i < count; i++)
    if ((int)st[(size_t)i * TOG_NSTATS + TOG_STAT_FLAGS] & TOG_TRAJ_ACTIVE)
      return fail(TOG_ERR_ARG, "tog_refill: slot " + std::to_string(slots[i]) + " is active");
  const long long first = h->jobs_started;
  rc = refill_enqueue(
      h, count, slots, [](int i) { return (long long)i; }, [&](int i) { return first + i; }, x0, U, X, nullptr,
      nullptr, nullptr);
  if (rc) return rc;
  h->jobs_started += count;
  HIPCHECK(hipStreamSynchronize(h->stream));  // the caller's arrays and the pinned staging are free again
  h->refill_pending = false;
  return TOG_OK;
}

int32_t tog_refill_tables(tog_handle* h, int32_t count, const int32_t* slots, const double* lin, const double* term,
                          const double* xf) {
  int32_t rc = stream_refuse(h, "tog_refill_tables");
  if (rc || (rc = obs_refuse(h, "tog_refill_tables"))) return rc;
  if ((rc = tables_check(h, lin, term, xf, "tog_refill_tables"))) return rc;
  if ((rc = check_slots(h, count, slots, true, "tog_refill_tables"))) return rc;
  if (count == 0 || (!lin && !term && !xf)) return TOG_OK;
  HIPCHECK(hipSetDevice(h->device));
  if ((rc = stream_alloc(h))) return rc;
  // (x0 null: the tables only; k_refill follows with tog_refill)
  rc = refill_enqueue(
      h, count, slots, [](int i) { return (long long)i; }, [](int) { return 0LL; }, nullptr, nullptr, nullptr, lin,
      term, xf);
  if (rc) return rc;
  HIPCHECK(hipStreamSynchronize(h->stream));
  h->refill_pending = false;
  return TOG_OK;
}

int32_t tog_solve_stream(tog_handle* h, int32_t mode, int64_t njobs, const double* x0, const double* U0, double* X_out,
                         double* U_out, double* stats_out, int32_t max_steps, int64_t* jobs_done) {
  if (int32_t rc = obs_refuse(h, "tog_solve_stream")) return rc;
  if (h && !is_multi(h) && (h->d_lin || h->d_term || h->d_goal))
    return fail(TOG_ERR_ARG, "tog_solve_stream: the handle has per-trajectory cost or goal tables; give every job its "
                             "rows through tog_solve_stream_tables");
  return solve_stream(h, mode, njobs, x0, U0, nullptr, nullptr, nullptr, X_out, U_out, stats_out, max_steps, jobs_done,
                      "tog_solve_stream");
}

int32_t tog_solve_stream_tables(tog_handle* h, int32_t mode, int64_t njobs, const double* x0, const double* U0,
                                const double* lin, const double* term, const double* xf, double* X_out, double* U_out,
                                double* stats_out, int32_t max_steps, int64_t* jobs_done) {
  int32_t rc = stream_refuse(h, "tog_solve_stream_tables");
  if (rc || (rc = obs_refuse(h, "tog_solve_stream_tables"))) return rc;
  if (!h->d_lin && !h->d_term && !h->d_goal)
    return fail(TOG_ERR_UNSUPPORTED, "tog_solve_stream_tables: the handle has no per-trajectory table (set them with "
                                     "tog_set_trajectory_costs / tog_set_trajectory_goals first; their kernel "
                                     "variants are chosen then)");
  if ((rc = tables_check(h, lin, term, xf, "tog_solve_stream_tables"))) return rc;
  if (njobs > 0 && ((h->d_lin && !lin) || (h->d_term && !term) || (h->d_goal && !xf)))
    return fail(TOG_ERR_ARG, "tog_solve_stream_tables: every table the handle has needs the jobs' rows");
  return solve_stream(h, mode, njobs, x0, U0, lin, term, xf, X_out, U_out, stats_out, max_steps, jobs_done,
                      "tog_solve_stream_tables");
}

static_assert((int)TOG_ROLLOUT_TAIL3 == (int)tog_plan::SPEC_TAIL3 && (int)TOG_ROLLOUT_TAIL1 == (int)tog_plan::SPEC_TAIL1 &&
                  (int)TOG_ROLLOUT_BULK == (int)tog_plan::SPEC_BULK &&
                  (int)TOG_ROLLOUT_BULK_W1 == (int)tog_plan::SPEC_BULK_W1,
              "tog_rollout_kernel mirrors tog_plan::SpecKernel");

int32_t tog_rollout_plan(tog_handle* h, int32_t cnt, int32_t listed, int32_t* kernel_out) {
  if (!h || !kernel_out) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) return tog_rollout_plan(h->parts[0], cnt, listed, kernel_out);  // (the parts share their flags)
  const DevBuffers& b = h->buf;
  if (cnt < 1 || cnt > b.nc) return fail(TOG_ERR_ARG, "tog_rollout_plan: cnt outside [1, iterations_linesearch + 1]");
  // the arguments ModelLaunch::spec passes (tog_launch.hpp)
  *kernel_out = (int32_t)tog_plan::spec_kernel(b.tail, b.cand ? 1 : 0, b.cost_diag, b.tv, listed != 0, cnt,
                                                b.spec_tail2_shmem, b.spec_tail_shmem, h->ops->n * h->ops->m);
  return TOG_OK;
}

int32_t tog_profile(tog_handle* h, int32_t enable) {
  if (!h) return fail(TOG_ERR_ARG, "null handle");
  if (is_multi(h)) return each_part(h, [&](tog_handle* p, size_t) { return tog_profile(p, enable); });
  HIPCHECK(hipSetDevice(h->device));
  if (enable) {
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->ev_used = 0;
    h->ev_kind.clear();
  }
  h->profiling = enable != 0;
  return TOG_OK;
}

int32_t tog_profile_read(tog_handle* h, double* total_ms, int64_t* launches) {
  if (!h || !total_ms || !launches) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) {  // summed over devices
    double ms[TOG_NKERNELS] = {0};
    int64_t ln[TOG_NKERNELS] = {0};
    int32_t rc = each_part(h, [&](tog_handle* p, size_t) {
      double a[TOG_NKERNELS];
      int64_t b[TOG_NKERNELS];
      int32_t r = tog_profile_read(p, a, b);
      for (int i = 0; i < TOG_NKERNELS; i++) ms[i] += a[i], ln[i] += b[i];
      return r;
    });
    for (int i = 0; i < TOG_NKERNELS; i++) total_ms[i] = ms[i], launches[i] = ln[i];
    return rc;
  }
  HIPCHECK(hipSetDevice(h->device));
  HIPCHECK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < TOG_NKERNELS; i++) {
    total_ms[i] = 0.0;
    launches[i] = 0;
  }
  for (size_t p = 0; p < h->ev_kind.size(); p++) {
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, h->ev_pool[2 * p], h->ev_pool[2 * p + 1]));
    total_ms[h->ev_kind[p]] += ms;
    launches[h->ev_kind[p]] += 1;
  }
  return TOG_OK;
}

void tog_default_pn_options(tog_pn_options* o) {
  o->n_steps = 1;
  o->solve_type = 0;
  o->active_set_tolerance = 1e-3;
  o->feasibility_tolerance = 1e-6;
}

// solve!(prob, ProjectedNewtonSolver) (projected_newton.jl:6-20): per newton step, k_pn_begin
// (update! + the first viol), then projection_solve!'s loop of at most 10 _projection_solve!s (each
// after k_jacobian at the current X, U), then k_pn_finish (record_iteration!). Trajectories that
// are done return at once from every launch.
int32_t tog_solve_pn(tog_handle* h, const tog_pn_options* opts, double* out) {
  if (!h || !opts) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h))
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_solve_pn(p, opts, out ? out + o * TOG_PN_NSTATS : nullptr);
    });
  if (opts->solve_type != 0 && opts->solve_type != 1) return fail(TOG_ERR_ARG, "solve_type must be 0 (:feasible) or 1 (:optimal)");
  if (h->d_lin || h->d_term || h->d_goal)
    return fail(TOG_ERR_UNSUPPORTED, "tog_solve_pn: per-trajectory costs or goals are set (projected Newton reads the "
                                     "shared objective and goal; clear them with NULL tables first)");
  if (h->d_obs) return fail(TOG_ERR_UNSUPPORTED, tog_traj::obstacles_set_text("tog_solve_pn"));
  if (h->d_bnd) return fail(TOG_ERR_UNSUPPORTED, tog_traj::bounds_set_text("tog_solve_pn"));
  if (h->d_hess) return fail(TOG_ERR_UNSUPPORTED, tog_traj::weights_set_text("tog_solve_pn"));
  const bool optimal = opts->solve_type == 1;
  if (opts->n_steps < 0) return fail(TOG_ERR_ARG, "n_steps must be >= 0");
  if (!h->ops->pn) return fail(TOG_ERR_UNSUPPORTED, "projected Newton needs n + m <= 64 (a lane per variable of a knot)");
  // block stride of the first pass: n + every row of a knot, capped at a wave's 64 rows; blocks are sized by the
  // *active* rows. A trajectory whose active set outgrows that stride stops there (PNState::over) and is solved
  // again below with the wide kernels (pn_solve_wide: strides up to 128 rows, which no built-in model exceeds),
  // so every problem whose blocks stay within 64 rows runs what it always ran
  const int SM = std::min(h->n + h->pmax, PN_SM_MAX);
  const bool may_widen = h->n + h->pmax > PN_SM_MAX;
  if (SM < h->n) return fail(TOG_ERR_UNSUPPORTED, "projected Newton needs n <= 64");
  HIPCHECK(hipSetDevice(h->device));
  {
    size_t lim = 0;
    const int32_t rl = pn_lds_limit(h, &lim);
    if (rl) return rl;
    const size_t lds = pn_lds_bytes(SM, h->n + h->m);
    if (lds > lim)
      return fail(TOG_ERR_UNSUPPORTED, "projected Newton's kernels need " + std::to_string(lds) +
                                           " bytes of LDS a workgroup; the device offers " + std::to_string(lim));
  }
  PNBuffers& W = h->pn;
  const long long B = h->B;
  if (h->pn_alloc && W.SM != SM) return fail(TOG_ERR_ARG, "projected Newton workspace stride changed");
  if (!h->pn_alloc) {
    W.SM = SM;
    W.nb = h->N + 1;
    const size_t blk = (size_t)B * W.nb * SM * SM, vec = (size_t)B * W.nb * SM;
    const size_t pm = (size_t)(h->pmax > 0 ? h->pmax : 1);
    // the whole workspace is sized before any allocation: a batch whose block factors do not fit the
    // device's free memory is refused with TOG_ERR_NOMEM (solve it in slices, tog_create_multi)
    const size_t nsnapX = may_widen ? (size_t)B * h->N * h->n : 0, nsnapU = may_widen ? (size_t)B * (h->N - 1) * h->m : 0;
    const size_t need = sizeof(double) * (4 * blk + 5 * vec + 2 * (size_t)B * h->N * h->n + nsnapX + nsnapU) +
                        sizeof(int) * ((size_t)B * h->N * pm + (size_t)B * h->N + (size_t)B * W.nb + (may_widen ? 2 * (size_t)B : 0)) +
                        sizeof(PNState) * (size_t)B;
    size_t fr = 0, tot = 0;
    HIPCHECK(hipMemGetInfo(&fr, &tot));
    if (need > fr)
      return fail(TOG_ERR_NOMEM, "projected Newton workspace (" + std::to_string(need >> 20) + " MiB) exceeds free device memory (" +
                                     std::to_string(fr >> 20) + " MiB)");
    const size_t mark = h->allocs.size();
    int rc;
    if ((rc = dalloc(h, &W.Sd, blk)) || (rc = dalloc(h, &W.So, blk)) || (rc = dalloc(h, &W.Ld, blk)) ||
        (rc = dalloc(h, &W.Lo, blk)) || (rc = dalloc(h, &W.yv, vec)) || (rc = dalloc(h, &W.xv, vec)) ||
        (rc = dalloc(h, &W.rv, vec)) || (rc = dalloc(h, &W.wv, vec)) || (rc = dalloc(h, &W.dv, vec)) ||
        (rc = dalloc(h, &W.yd, (size_t)B * h->N * h->n)) || (rc = dalloc(h, &W.Xs, (size_t)B * h->N * h->n)) ||
        (rc = dalloc(h, &W.act, (size_t)B * h->N * (h->pmax > 0 ? h->pmax : 1))) ||
        (rc = dalloc(h, &W.na, (size_t)B * h->N)) || (rc = dalloc(h, &W.sz, (size_t)B * W.nb)) ||
        (rc = dalloc(h, &W.st, (size_t)B)) ||
        (may_widen && ((rc = dalloc(h, &h->pn_X0, nsnapX)) || (rc = dalloc(h, &h->pn_U0, nsnapU)) ||
                       (rc = dalloc(h, &h->pn_slot_of, (size_t)B)) || (rc = dalloc(h, &h->pn_park, (size_t)B)))) ||
        (h->ops->min_time && (rc = dalloc(h, &W.wt, (size_t)B * ((size_t)h->N * h->n + (size_t)(h->N - 1) * h->m))))) {
      // partial failure: release what this call allocated, so a retry does not leak it
      for (size_t i = mark; i < h->allocs.size(); i++) (void)hipFree(h->allocs[i]);
      h->allocs.resize(mark);
      (void)hipGetLastError();
      return rc;
    }
    h->pn_alloc = true;
  }
  if (optimal && !h->pn_opt_alloc) {  // :optimal's workspace: two more block factors, the duals and the KKT vectors
    const size_t blk = (size_t)B * W.nb * SM * SM, vec = (size_t)B * W.nb * SM;
    const size_t nz = (size_t)B * h->N * (h->n + h->m), nx = (size_t)B * h->N * h->n;
    const size_t nc = (size_t)B * h->N * (h->pmax > 0 ? h->pmax : 1), nu = (size_t)B * (h->N - 1) * h->m;
    const size_t need = sizeof(double) * (2 * blk + 2 * vec + 3 * nz + 4 * nx + 3 * nc + nu) + sizeof(int) * (size_t)B * W.nb;
    size_t fr = 0, tot = 0;
    HIPCHECK(hipMemGetInfo(&fr, &tot));
    if (need > fr)
      return fail(TOG_ERR_NOMEM, "projected Newton :optimal workspace (" + std::to_string(need >> 20) +
                                     " MiB) exceeds free device memory (" + std::to_string(fr >> 20) + " MiB)");
    const size_t mark = h->allocs.size();
    int rc;
    if ((rc = dalloc(h, &W.Ld2, blk)) || (rc = dalloc(h, &W.Lo2, blk)) || (rc = dalloc(h, &W.lb, vec)) ||
        (rc = dalloc(h, &W.tb, vec)) || (rc = dalloc(h, &W.g, nz)) || (rc = dalloc(h, &W.rz, nz)) ||
        (rc = dalloc(h, &W.dz, nz)) || (rc = dalloc(h, &W.nu, nx)) || (rc = dalloc(h, &W.dnu, nx)) ||
        (rc = dalloc(h, &W.nut, nx)) || (rc = dalloc(h, &W.Xv, nx)) || (rc = dalloc(h, &W.lc, nc)) ||
        (rc = dalloc(h, &W.dlc, nc)) || (rc = dalloc(h, &W.lct, nc)) || (rc = dalloc(h, &W.Uv, nu)) ||
        (rc = dalloc(h, &W.szS, (size_t)B * W.nb))) {
      for (size_t i = mark; i < h->allocs.size(); i++) (void)hipFree(h->allocs[i]);
      h->allocs.resize(mark);
      (void)hipGetLastError();
      return rc;
    }
    h->pn_opt_alloc = true;
  }
  W.optimal = optimal ? 1 : 0;
  if (optimal) {  // PrimalDual(prob): zero duals
    HIPCHECK(hipMemsetAsync(W.nu, 0, sizeof(double) * (size_t)B * h->N * h->n, h->stream));
    HIPCHECK(hipMemsetAsync(W.lc, 0, sizeof(double) * (size_t)B * h->N * (h->pmax > 0 ? h->pmax : 1), h->stream));
  }
  W.atol = opts->active_set_tolerance;
  W.eps = opts->feasibility_tolerance;
  HIPCHECK(hipMemsetAsync(W.st, 0, sizeof(PNState) * B, h->stream));
  // solver_pn.stats[:cost] / [:c_max] per newton step (tog_get_pn_history): read after each step's
  // record_iteration! (k_pn_finish); a trajectory records in a step iff its step counter moved
  h->pn_hist.assign((size_t)2 * std::max(opts->n_steps, 0) * B, NAN);
  h->pn_hist_steps = opts->n_steps;
  if (may_widen && opts->n_steps > 0) {  // the wide pass restarts from here (a later newton step may be the one that overflows)
    HIPCHECK(hipMemcpyAsync(h->pn_X0, h->buf.X, sizeof(double) * (size_t)B * h->N * h->n, hipMemcpyDeviceToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->pn_U0, h->buf.U, sizeof(double) * (size_t)B * (h->N - 1) * h->m, hipMemcpyDeviceToDevice, h->stream));
  }
  std::vector<PNState> stp, stw;
  int32_t rc = pn_pass(h, opts, optimal, W.st, B, stp,
                       [&](int phase) { return h->ops->pn(h->dP, h->buf, W, B, h->integ, phase, h->stream); },
                       [](long long s) { return s; });
  if (rc) return rc;
  // the trajectories the narrow pass stopped on a block above its stride: again, with the wide kernels
  std::vector<int> wide;
  if (may_widen && opts->n_steps > 0)
    for (long long b = 0; b < B; b++)
      if (stp[b].over) wide.push_back((int)b);
  if (!wide.empty() && (rc = pn_solve_wide(h, opts, optimal, wide, stw))) return rc;
  h->pn_hist_rec.assign(B, 0);
  for (long long b = 0; b < B && opts->n_steps > 0; b++) h->pn_hist_rec[b] = stp[b].steps;
  for (size_t s = 0; s < wide.size(); s++) h->pn_hist_rec[wide[s]] = stw[s].steps;
  if (out) {
    std::vector<PNState> st(B);
    HIPCHECK(hipMemcpyAsync(st.data(), W.st, sizeof(PNState) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    for (size_t s = 0; s < wide.size(); s++) st[wide[s]] = stw[s];
    for (long long b = 0; b < B; b++) {
      double* o = out + b * TOG_PN_NSTATS;
      o[TOG_PN_VIOL] = st[b].viol;
      o[TOG_PN_C_MAX] = st[b].c_max;
      o[TOG_PN_J] = st[b].J;
      o[TOG_PN_PROJECTIONS] = st[b].projections;
      o[TOG_PN_LINESEARCHES] = st[b].linesearches;
      o[TOG_PN_REFINEMENTS] = st[b].refinements;
      o[TOG_PN_STEPS] = st[b].steps;
    }
  }
  return TOG_OK;
}

int32_t tog_get_pn_history(tog_handle* h, double* out, int32_t* steps_out) {
  if (!h || !out) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) {
    const size_t w = 2 * (size_t)std::max(h->parts[0]->pn_hist_steps, 0);
    return each_part(h, [&](tog_handle* p, size_t o) {
      return tog_get_pn_history(p, out + o * w, steps_out ? steps_out + o : nullptr);
    });
  }
  if (h->pn_hist_steps < 0) return fail(TOG_ERR_ARG, "no projected Newton solve on this handle");
  std::copy(h->pn_hist.begin(), h->pn_hist.end(), out);
  if (steps_out)
    for (long long b = 0; b < h->B; b++) steps_out[b] = h->pn_hist_rec.empty() ? 0 : h->pn_hist_rec[b];
  return TOG_OK;
}

int32_t tog_status(tog_handle* h, int32_t* flags_out) {
  if (!h || !flags_out) return fail(TOG_ERR_ARG, "null argument");
  if (is_multi(h)) return each_part(h, [&](tog_handle* p, size_t o) { return tog_status(p, flags_out + o); });
  std::vector<TrajState> st;
  int rc = get_states(h, st);
  if (rc) return rc;
  for (size_t i = 0; i < st.size(); i++) flags_out[i] = st[i].flags | (st[i].active ? TOG_TRAJ_ACTIVE : 0);
  return TOG_OK;
}

// (internal, diagnostics) the last forward pass's speculative trials: J (nc, B) and rollout status (nc, B)
int32_t tog__debug_ls(tog_handle* h, double* J, int32_t* ok, int32_t* nc) {
  if (!h || is_multi(h)) return fail(TOG_ERR_ARG, "tog__debug_ls: single-device handle");
  *nc = h->buf.nc;
  HIPCHECK(hipStreamSynchronize(h->stream));
  if (J) HIPCHECK(hipMemcpy(J, h->buf.lsJ, sizeof(double) * h->buf.nc * h->B, hipMemcpyDeviceToHost));
  if (ok) HIPCHECK(hipMemcpy(ok, h->buf.lsok, sizeof(int) * h->buf.nc * h->B, hipMemcpyDeviceToHost));
  return TOG_OK;
}

}  // extern "C"
