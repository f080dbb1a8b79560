// Host side of the per-trajectory cost and goal tables (tog_set_trajectory_costs / tog_set_trajectory_goals,
// include/tog.h): argument checks, the host images of the device tables, the slices a multi-device handle hands
// to its parts, and the replace order of a device buffer (and of tog_history_enable's pair). Plain C++ with no device runtime in it, so that a
// stand-alone program can run it under the host sanitizers (tests/c/traj_tables_host.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "tog_host_plan.hpp"  // chol_upper, factor_stage, cost_class: the per-trajectory weights' factors and class

namespace tog_traj {

// doubles per trajectory of the three host arrays
inline size_t lin_width(int n, int m, int N, int per_knot) {
  return (size_t)(n + m + 1) * (per_knot ? (size_t)(N - 1) : 1);
}
inline size_t term_width(int n) { return (size_t)n + 1; }

// The terminal knot's goal rows. types / idx: every row's type and state index, knot_off / knot_cnt the rows of
// each knot; goal_type the goal row type. Fills goal_idx with the state index of each terminal goal row in row
// order (ng = its size). An error text when a goal row sits at a stage knot or two terminal goal rows share a
// state (the device table is indexed by state), else empty.
inline std::string terminal_goal_rows(const int* types, const int* idx, const int* knot_off, const int* knot_cnt,
                                      int N, int n, int goal_type, std::vector<int>& goal_idx) {
  goal_idx.clear();
  std::vector<char> seen((size_t)n, 0);
  for (int k = 0; k < N; k++)
    for (int r = 0; r < knot_cnt[k]; r++) {
      const int row = knot_off[k] + r;
      if (types[row] != goal_type) continue;
      if (k != N - 1) return "per-trajectory goals: a goal row at stage knot " + std::to_string(k);
      const int i = idx[row];
      if (i < 0 || i >= n) return "per-trajectory goals: goal row state index out of range";
      if (seen[(size_t)i]) return "per-trajectory goals: two terminal goal rows on state " + std::to_string(i);
      seen[(size_t)i] = 1;
      goal_idx.push_back(i);
    }
  return std::string();
}

// (ng, B) goal values -> the device table's host image (n, B): entry (goal_idx[j], b) = xf[j + ng b]; states
// without a goal row stay 0 (never read)
inline std::vector<double> goal_table(const double* xf, const std::vector<int>& goal_idx, int n, long long B) {
  const size_t ng = goal_idx.size();
  std::vector<double> t((size_t)n * (size_t)B, 0.0);
  for (long long b = 0; b < B; b++)
    for (size_t j = 0; j < ng; j++) t[(size_t)b * n + (size_t)goal_idx[j]] = xf[(size_t)b * ng + j];
  return t;
}

// one per-knot cost row (kst doubles) repeated for the N - 1 stage knots: the per-knot table of a handle whose
// descriptor had a single stage cost (cost_at reads the per-trajectory terms beside a per-knot table)
inline std::vector<double> replicate_row(const std::vector<double>& row, int knots) {
  std::vector<double> t(row.size() * (size_t)knots);
  for (int k = 0; k < knots; k++) memcpy(t.data() + (size_t)k * row.size(), row.data(), sizeof(double) * row.size());
  return t;
}

// ---- per-trajectory obstacles (tog_set_trajectory_obstacles): the data of the circle and sphere rows.
// Every obstacle of every circles / spheres constraint in the descriptor's sets table has an ordinal: sets in
// order, constraints in their set's order, obstacles in their constraint's order. A set used at many knots (or at
// none) contributes once. set_ncon[s]: constraints of set s; con_type / con_count: type and obstacle count of
// each constraint, all sets' constraints in one run. base[i]: the ordinal of constraint i's first obstacle (-1:
// not an obstacle constraint); kind[j]: 0 for a circle, 1 for a sphere. Returns no, the number of ordinals.
inline int obstacle_ordinals(const int* set_ncon, int n_sets, const int* con_type, const int* con_count,
                             int circles_type, int spheres_type, std::vector<int>& base, std::vector<char>& kind) {
  base.clear();
  kind.clear();
  int i = 0, no = 0;
  for (int s = 0; s < n_sets; s++)
    for (int c = 0; c < set_ncon[s]; c++, i++) {
      const bool obs = con_type[i] == circles_type || con_type[i] == spheres_type;
      const int cnt = obs && con_count[i] > 0 ? con_count[i] : 0;
      base.push_back(obs ? no : -1);
      kind.insert(kind.end(), (size_t)cnt, con_type[i] == spheres_type ? 1 : 0);
      no += cnt;
    }
  return no;
}
// doubles per trajectory of the obstacle array, and of the device table (DevProblem::obs_ld)
inline size_t obs_width(int no) { return 4 * (size_t)no; }
// (4, no, B) -> the device table's host image, the same layout: entry (., j, b) = [x0, y0, z0, r], with the
// unused third number of a circle stored as 0
inline std::vector<double> obstacle_table(const double* obs, const std::vector<char>& kind, long long B) {
  const size_t no = kind.size();
  std::vector<double> t(obs, obs + obs_width((int)no) * (size_t)B);
  for (long long b = 0; b < B; b++)
    for (size_t j = 0; j < no; j++)
      if (!kind[j]) t[((size_t)b * no + j) * 4 + 2] = 0.0;
  return t;
}
inline std::string obstacles_none_text() {
  return "tog_set_trajectory_obstacles: the problem has no circle or sphere constraint";
}
// infeasible-start and minimum-time handles
inline std::string obstacles_refuse_text() {
  return "tog_set_trajectory_obstacles: infeasible-start and minimum-time problems keep the batch's obstacles "
         "(their augmented rows are built from the descriptor)";
}
// the entry points whose kernels or staging read the descriptor's obstacle data
inline std::string obstacles_set_text(const char* who) {
  return std::string(who) + ": per-trajectory obstacles are set (this call reads the descriptor's circle and sphere "
                            "data; clear the table with tog_set_trajectory_obstacles(h, NULL) first)";
}

// ---- per-trajectory bounds (tog_set_trajectory_bounds): the limit `a` of the bound rows.
// Every bound row that build_rows keeps over the descriptor's sets table has an ordinal: sets in order,
// constraints in their set's order, within a bound constraint the kept rows in the order [x_max; u_max; x_min;
// u_min]. A set used at many knots (or at none) contributes once; a set that only the terminal knot uses
// contributes no control rows (the terminal knot has none). The row keeps its ordinal in ConRow::b.
// u_kept: whether build_rows keeps the control row i of a bound constraint at a stage knot, finiteness aside
// (keep: trim = false; slack, mt: the slack controls and the time step of an infeasible-start / minimum-time
// problem, which an untrimmed bound leaves out or adds)
inline bool bound_u_kept(int i, bool keep, int m, int slack, int mt) {
  const int mb = keep ? m - slack - mt : m;
  return i < mb || (keep && mt && i == m - 1);
}
struct BoundPlan {
  // per constraint (all sets' constraints in one run): the ordinal of the first kept row of each block
  // [x_max, u_max, x_min, u_min] (-1: not a bound constraint)
  std::vector<int> base;
  std::vector<char> trimmed;  // per ordinal: 1 when the row exists because its bound is finite (a trimmed constraint)
  int nb = 0;
};
// set_ncon[s]: constraints of set s; set_term[s]: 1 when only the terminal knot uses set s; con_type /
// con_count / con_data: type, count (0: trim = true, 1: trim = false) and data [x_max(n), x_min(n), u_max(m),
// u_min(m)] of each constraint. Returns nb.
inline int bound_ordinals(const int* set_ncon, const char* set_term, int n_sets, const int* con_type,
                          const int* con_count, const double* const* con_data, int bound_type, int n, int m,
                          int slack, int mt, BoundPlan& plan) {
  plan.base.clear();
  plan.trimmed.clear();
  int i = 0, nb = 0;
  auto finite = [](double v) { return v == v && v - v == 0.0; };
  for (int s = 0; s < n_sets; s++)
    for (int c = 0; c < set_ncon[s]; c++, i++) {
      if (con_type[i] != bound_type) {
        plan.base.insert(plan.base.end(), 4, -1);
        continue;
      }
      const bool keep = con_count[i] == 1;
      const double* D = con_data[i];
      // block order [x_max; u_max; x_min; u_min]; data offsets 0, 2n, n, 2n + m
      const int off[4] = {0, 2 * n, n, 2 * n + m};
      for (int blk = 0; blk < 4; blk++) {
        const bool isu = blk & 1;
        plan.base.push_back(nb);
        if (isu && set_term[s]) continue;
        for (int j = 0; j < (isu ? m : n); j++) {
          if (isu && !bound_u_kept(j, keep, m, slack, mt)) continue;
          if (!keep && !finite(D[off[blk] + j])) continue;
          plan.trimmed.push_back(keep ? 0 : 1);
          nb++;
        }
      }
    }
  plan.nb = nb;
  return nb;
}
// (nb, B) limits: empty when they can replace the rows' own, else why not. A NaN anywhere, or a non-finite value
// at a row of a trimmed constraint (the row exists because the bound is finite; an untrimmed row may be
// infinite, as in the descriptor).
inline std::string bound_table_check(const double* bnd, const std::vector<char>& trimmed, long long B) {
  const size_t nb = trimmed.size();
  for (long long b = 0; b < B; b++)
    for (size_t j = 0; j < nb; j++) {
      const double v = bnd[(size_t)b * nb + j];
      if (v != v)
        return "tog_set_trajectory_bounds: NaN at row " + std::to_string(j) + " of trajectory " + std::to_string(b);
      if (trimmed[j] && v - v != 0.0)
        return "tog_set_trajectory_bounds: infinite bound at row " + std::to_string(j) + " of trajectory " +
               std::to_string(b) + " (a row of a trimmed constraint exists because its bound is finite)";
    }
  return std::string();
}
inline std::string bounds_none_text() { return "tog_set_trajectory_bounds: the problem has no bound row"; }
// infeasible-start and minimum-time handles
inline std::string bounds_refuse_text() {
  return "tog_set_trajectory_bounds: infeasible-start and minimum-time problems keep the batch's bounds (their "
         "combined bounds are built from the descriptor)";
}
// the entry points whose kernels or staging read the descriptor's bounds
inline std::string bounds_set_text(const char* who) {
  return std::string(who) + ": per-trajectory bounds are set (this call reads the descriptor's bounds; clear the "
                            "table with tog_set_trajectory_bounds(h, NULL) first)";
}

// ---- per-trajectory cost weights (tog_set_trajectory_weights): the Hessians Q, R, H and Qf of each trajectory.
// The host array W is (nw, B): per trajectory [Q (n, n); R (m, m); H (m, n); Qf (n, n)], matrices column-major with
// the compact n, m. The device table (DevProblem::hess) is (nh, B): per trajectory [Q; R; H; cQ; cR; Qf; cQf] with
// cQ = chol(Q dt), cR = chol(R dt), cQf = chol(Qf), the factors tog_create computes for the shared cost
// (tog_plan::factor_stage, chol_upper), so a member's block is bit for bit what a handle of its own would hold.
inline size_t weights_width(int n, int m) { return 2 * (size_t)n * n + (size_t)m * m + (size_t)m * n; }
inline size_t hess_width(int n, int m) { return 4 * (size_t)n * n + 2 * (size_t)m * m + (size_t)m * n; }
// offsets of the blocks in a trajectory's device image
struct HessLayout {
  int R, H, cQ, cR, Qf, cQf, nh;
  constexpr HessLayout(int n, int m)
      : R(n * n), H(R + m * m), cQ(H + m * n), cR(cQ + n * n), Qf(cR + m * m), cQf(Qf + n * n), nh(cQf + n * n) {}
};
struct WeightPlan {
  std::vector<double> image;  // (nh, B)
  bool sqrt_ok = true;        // every trajectory's Hessians are PD (the AND over the batch)
  int diag_cost = 2;          // the minimum over the batch of tog_plan::cost_class
  // the first Hessian that is not positive definite, in the order tog_create factors them (Qf, Q, R): its
  // trajectory (-1: none) and its name
  long long bad_traj = -1;
  const char* bad_mat = "";
};
// (nw, B) weights: empty when they can replace the shared Hessians, else why not: a NaN or an infinity, or a Q, R
// or Qf that is not symmetric. The message names the trajectory and the matrix. (Positive definiteness, which a
// square-root handle asks for, is weight_plan's finding: the factors are computed once, there.)
inline std::string weight_table_check(const double* W, int n, int m, long long B) {
  const size_t nw = weights_width(n, m);
  const char* names[4] = {"Q", "R", "H", "Qf"};
  const int dims[4][2] = {{n, n}, {m, m}, {m, n}, {n, n}};
  for (long long b = 0; b < B; b++) {
    const double* w = W + (size_t)b * nw;
    const double* mat[4] = {w, w + n * n, w + n * n + m * m, w + n * n + m * m + m * n};
    for (int k = 0; k < 4; k++) {
      const int rows = dims[k][0], cols = dims[k][1];
      for (int i = 0; i < rows * cols; i++)
        if (mat[k][i] - mat[k][i] != 0.0)  // (NaN or infinite)
          return "tog_set_trajectory_weights: trajectory " + std::to_string(b) + ": " + names[k] +
                 " has a NaN or an infinite entry";
      if (k == 2) continue;
      for (int j = 0; j < cols; j++)
        for (int i = 0; i < j; i++)
          if (mat[k][i + rows * j] != mat[k][j + rows * i])
            return "tog_set_trajectory_weights: trajectory " + std::to_string(b) + ": " + names[k] +
                   " is not symmetric";
    }
  }
  return std::string();
}
// the device table's host image with the batch's sqrt_ok and diagonal-cost class
inline WeightPlan weight_plan(const double* W, int n, int m, double dt, long long B) {
  const size_t nw = weights_width(n, m);
  const HessLayout L(n, m);
  WeightPlan p;
  p.image.assign((size_t)L.nh * (size_t)B, 0.0);
  for (long long b = 0; b < B; b++) {
    const double* w = W + (size_t)b * nw;
    const double *Q = w, *R = w + n * n, *H = R + m * m, *Qf = H + m * n;
    double* o = p.image.data() + (size_t)b * L.nh;
    memcpy(o, Q, sizeof(double) * n * n);
    memcpy(o + L.R, R, sizeof(double) * m * m);
    memcpy(o + L.H, H, sizeof(double) * m * n);
    memcpy(o + L.Qf, Qf, sizeof(double) * n * n);
    const bool okf = tog_plan::chol_upper(Qf, n, o + L.cQf);
    const int st = tog_plan::factor_stage(n, m, dt, Q, R, o + L.cQ, o + L.cR);
    const bool ok = okf && st == 0;
    if (!ok && p.bad_traj < 0) {
      p.bad_traj = b;
      p.bad_mat = !okf ? "Qf" : (st == 1 ? "Q" : "R");
    }
    p.sqrt_ok = p.sqrt_ok && ok;
    p.diag_cost = std::min(p.diag_cost, tog_plan::cost_class(n, m, dt, Q, R, H, Qf, o + L.cQ, o + L.cR, o + L.cQf, ok));
  }
  return p;
}
// a square-root handle's refusal of a plan whose Hessians are not all positive definite (empty: they are)
inline std::string weight_pd_text(const WeightPlan& p) {
  if (p.sqrt_ok) return std::string();
  return "tog_set_trajectory_weights: trajectory " + std::to_string(p.bad_traj) + ": " + p.bad_mat +
         " is not positive definite (the sqrt backward pass, objective.jl:70-94)";
}
// a handle whose descriptor came with a time-varying stage_costs table
inline std::string weights_varying_text() {
  return "tog_set_trajectory_weights: the problem has a time-varying stage_costs table (cost Hessians per "
         "trajectory and per knot are not built)";
}
// the entry points whose kernels or staging read the descriptor's Hessians
inline std::string weights_set_text(const char* who) {
  return std::string(who) + ": per-trajectory cost weights are set (this call reads the descriptor's cost Hessians; "
                            "clear the table with tog_set_trajectory_weights(h, NULL) first)";
}

// a host array's slice for the part of a multi-device handle that starts at trajectory `off` (the batch axis is
// the outermost one; a null array stays null)
inline const double* part_slice(const double* a, size_t off, size_t width) { return a ? a + off * width : nullptr; }

// Replace a device buffer by a new one holding `count` doubles of `src`: the new buffer is allocated and filled
// first, and only then is the old one released and the slot updated, so a failure leaves the old table in place.
// alloc(count) -> pointer or null, upload(dst, src, count) -> bool, release(ptr).
template <class Alloc, class Upload, class Release>
inline bool replace_buffer(double** slot, const double* src, size_t count, Alloc&& alloc, Upload&& upload,
                           Release&& release) {
  double* fresh = alloc(count);
  if (!fresh) return false;
  if (!upload(fresh, src, count)) {
    release(fresh);
    return false;
  }
  double* old = *slot;
  *slot = fresh;
  if (old) release(old);
  return true;
}
// Replace two device buffers together by fresh ones of count_a and count_b doubles (contents undefined; the
// iteration histories of tog_history_enable). Both are allocated first: if either allocation fails, whatever was
// freshly allocated is released, both slots and the old buffers stay untouched, and it returns false. Otherwise
// the old ones are released and the slots updated.
template <class Alloc, class Release>
inline bool replace_buffer_pair(double** slot_a, size_t count_a, double** slot_b, size_t count_b, Alloc&& alloc,
                                Release&& release) {
  double* a = alloc(count_a);
  if (!a) return false;
  double* b = alloc(count_b);
  if (!b) {
    release(a);
    return false;
  }
  if (*slot_a) release(*slot_a);
  if (*slot_b) release(*slot_b);
  *slot_a = a;
  *slot_b = b;
  return true;
}
// back to the shared values: release the table (null: nothing)
template <class Release>
inline void drop_buffer(double** slot, Release&& release) {
  if (*slot) release(*slot);
  *slot = nullptr;
}

}  // namespace tog_traj
