// Stand-alone host check of the bound part of csrc/tog_traj_tables.hpp (the host side of
// tog_set_trajectory_bounds): the ordinals over a sets table, the count nb, the argument checks, the slices a
// multi-device handle hands to its parts and the error texts. Built with -fsanitize=address,undefined by
// tests/test_trajectory_bounds.py; it has no device code and needs no GPU. Exit status 0 and "ok" on success.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "tog_traj_tables.hpp"

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                               \
    }                                                        \
  } while (0)

int main() {
  using namespace tog_traj;
  const int BOUND = 0, GOAL = 1, CIRCLES = 2;  // (the values of include/tog.h's tog_constraint_type)
  const double inf = std::numeric_limits<double>::infinity();
  const int n = 3, m = 2;
  // data = [x_max(n), x_min(n), u_max(m), u_min(m)]
  const double u_only[10] = {inf, inf, inf, -inf, -inf, -inf, inf, inf, 0.1, -2.0};      // u_min rows only
  const double stage[10] = {0.5, 1.0, inf, -0.5, 0.0, -inf, 1.5, 1.5, 0.1, -2.0};        // heading trimmed
  const double circle[3] = {0.0, 0.0, 1.0};
  const double goal[3] = {0.0, 1.0, 0.0};

  // sets table: 0: [bound u-only] (knot 0)   1: [bound stage, circles] (stage knots)   2: [bound stage, goal]
  // (the terminal knot's: x rows only)   3: [bound stage, trim = false] (a set no knot uses still counts, with its
  // u rows)   4: []
  {
    const int ncon[5] = {1, 2, 2, 1, 0};
    const char term[5] = {0, 0, 1, 0, 0};
    const int type[6] = {BOUND, BOUND, CIRCLES, BOUND, GOAL, BOUND};
    const int count[6] = {0, 0, 1, 0, 3, 1};
    const double* data[6] = {u_only, stage, circle, stage, goal, stage};
    BoundPlan p;
    const int nb = bound_ordinals(ncon, term, 5, type, count, data, BOUND, n, m, 0, 0, p);
    CHECK(nb == 2 + 8 + 4 + 10 && p.nb == nb && p.trimmed.size() == (size_t)nb && p.base.size() == 24);
    // blocks [x_max, u_max, x_min, u_min] of each constraint
    const int want[24] = {0, 0, 0, 0, /* u-only: two u_min rows at 0, 1 */
                          2, 4, 6, 8,  /* stage */
                          -1, -1, -1, -1,
                          10, 12, 12, 14, /* terminal: x_max at 10, 11; x_min at 12, 13; no u rows */
                          -1, -1, -1, -1,
                          14, 17, 19, 22}; /* untrimmed: 3 + 2 + 3 + 2 */
    for (int i = 0; i < 24; i++) CHECK(p.base[i] == want[i]);
    for (int j = 0; j < nb; j++) CHECK(p.trimmed[j] == (j < 14 ? 1 : 0));

    // the argument checks over (nb, B): every element read, NaN anywhere, infinities at trimmed rows only
    const long long B = 5;
    std::vector<double> t((size_t)nb * B);
    for (size_t i = 0; i < t.size(); i++) t[i] = 1.0 + (double)i;
    CHECK(bound_table_check(t.data(), p.trimmed, B).empty());
    t[(size_t)4 * nb + 23] = inf;  // the last row of the last trajectory, untrimmed: allowed
    t[(size_t)2 * nb + 14] = -inf;
    CHECK(bound_table_check(t.data(), p.trimmed, B).empty());
    t[(size_t)3 * nb + 13] = inf;  // a trimmed row
    std::string e = bound_table_check(t.data(), p.trimmed, B);
    CHECK(e.find("infinite bound at row 13 of trajectory 3") != std::string::npos);
    t[(size_t)3 * nb + 13] = 1.0;
    t[(size_t)4 * nb + 20] = std::nan("");  // NaN at an untrimmed row
    e = bound_table_check(t.data(), p.trimmed, B);
    CHECK(e.find("NaN at row 20 of trajectory 4") != std::string::npos);
    t[(size_t)4 * nb + 20] = 2.0;
    t[0] = std::nan("");
    CHECK(bound_table_check(t.data(), p.trimmed, B).find("NaN at row 0 of trajectory 0") != std::string::npos);
    t[0] = 1.0;

    // multi-device split: B = 5 over parts of 3 and 2, each slice checked to its end
    const long long off[3] = {0, 3, 5};
    for (int q = 0; q < 2; q++) {
      const double* s = part_slice(t.data(), (size_t)off[q], (size_t)nb);
      CHECK(s == t.data() + (size_t)off[q] * nb);
      CHECK(bound_table_check(s, p.trimmed, off[q + 1] - off[q]).empty());
    }
    t[(size_t)4 * nb + 2] = std::nan("");  // seen by the second part as its trajectory 1
    CHECK(bound_table_check(part_slice(t.data(), 3, (size_t)nb), p.trimmed, 2).find("row 2 of trajectory 1") !=
          std::string::npos);
    CHECK(bound_table_check(part_slice(t.data(), 0, (size_t)nb), p.trimmed, 3).empty());
    CHECK(part_slice(nullptr, 3, (size_t)nb) == nullptr);
  }

  // a set that stage knots and the terminal knot share (a hand-written descriptor): not terminal-only, so its u
  // rows count and the terminal knot's x rows take the stage rows' ordinals
  {
    const int ncon[1] = {1};
    const char term[1] = {0};
    const int type[1] = {BOUND};
    const int count[1] = {0};
    const double* data[1] = {stage};
    BoundPlan p;
    CHECK(bound_ordinals(ncon, term, 1, type, count, data, BOUND, n, m, 0, 0, p) == 8);
    CHECK(p.base[0] == 0 && p.base[1] == 2 && p.base[2] == 4 && p.base[3] == 6);
  }

  // the control rows an untrimmed bound keeps on an infeasible-start problem (m = 2 + 3 slack controls: the
  // model's two) and on a minimum-time one (m = 3: the model's two and the time step, the last control)
  {
    CHECK(bound_u_kept(1, true, 5, 3, 0) && !bound_u_kept(2, true, 5, 3, 0) && bound_u_kept(4, false, 5, 3, 0));
    CHECK(bound_u_kept(1, true, 3, 0, 1) && bound_u_kept(2, true, 3, 0, 1));
    CHECK(bound_u_kept(0, true, 6, 3, 1) && bound_u_kept(1, true, 6, 3, 1) && !bound_u_kept(2, true, 6, 3, 1) &&
          !bound_u_kept(4, true, 6, 3, 1) && bound_u_kept(5, true, 6, 3, 1));
    const double d5[2 * 3 + 2 * 5] = {1, 1, 1, -1, -1, -1, 2, 2, inf, inf, inf, -2, -2, -inf, -inf, -inf};
    const int ncon[1] = {1};
    const char term[1] = {0};
    const int type[1] = {BOUND};
    const int keep[1] = {1}, trim[1] = {0};
    const double* data[1] = {d5};
    BoundPlan p;
    CHECK(bound_ordinals(ncon, term, 1, type, keep, data, BOUND, 3, 5, 3, 0, p) == 3 + 2 + 3 + 2);
    CHECK(bound_ordinals(ncon, term, 1, type, trim, data, BOUND, 3, 5, 3, 0, p) == 3 + 2 + 3 + 2);
    CHECK(p.base[1] == 3 && p.base[2] == 5 && p.base[3] == 8);
  }

  // no bound constraint, and an empty sets table
  {
    const int ncon[1] = {2};
    const char term[1] = {0};
    const int type[2] = {GOAL, CIRCLES};
    const int count[2] = {3, 1};
    const double* data[2] = {goal, circle};
    BoundPlan p;
    CHECK(bound_ordinals(ncon, term, 1, type, count, data, BOUND, n, m, 0, 0, p) == 0 && p.trimmed.empty());
    CHECK(p.base.size() == 8 && p.base[0] == -1 && p.base[7] == -1);
    CHECK(bound_ordinals(nullptr, nullptr, 0, nullptr, nullptr, nullptr, BOUND, n, m, 0, 0, p) == 0 && p.base.empty());
    CHECK(bound_table_check(nullptr, p.trimmed, 7).empty());
  }

  // error texts
  CHECK(bounds_none_text().find("no bound row") != std::string::npos);
  CHECK(bounds_refuse_text().find("infeasible-start and minimum-time") != std::string::npos);
  const std::string s = bounds_set_text("tog_refill");
  CHECK(s.rfind("tog_refill: per-trajectory bounds are set", 0) == 0);
  CHECK(s.find("tog_set_trajectory_bounds(h, NULL)") != std::string::npos);

  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
