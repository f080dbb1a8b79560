// Host side of the per-trajectory cost and goal tables (tog_set_trajectory_costs / tog_set_trajectory_goals,
// include/tog.h): argument checks, the host images of the device tables, the slices a multi-device handle hands
// to its parts, and the replace order of a device buffer (and of tog_history_enable's pair). Plain C++ with no device runtime in it, so that a
// stand-alone program can run it under the host sanitizers (tests/c/traj_tables_host.cpp).
#pragma once
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

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
