// Stand-alone host check of the obstacle part of csrc/tog_traj_tables.hpp (the host side of
// tog_set_trajectory_obstacles): the ordinals over a sets table, the count no, the table's host image, the slices a
// multi-device handle hands to its parts and the error texts. Built with -fsanitize=address,undefined by
// tests/test_trajectory_obstacles.py; it has no device code and needs no GPU. Exit status 0 and "ok" on success.
#include <cstdio>
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
  const int BOUND = 0, GOAL = 1, CIRCLES = 2, SPHERES = 3;  // (the values of include/tog.h's tog_constraint_type)

  // sets table: 0: [bound, circles x2, spheres x3]   1: [goal]   2: [spheres x1, bound, circles x1]   3: []
  // 4: [circles x2] (a set no knot uses still has ordinals: the count is over the table)
  {
    const int ncon[5] = {3, 1, 3, 0, 1};
    const int type[8] = {BOUND, CIRCLES, SPHERES, GOAL, SPHERES, BOUND, CIRCLES, CIRCLES};
    const int count[8] = {0, 2, 3, 4, 1, 1, 1, 2};
    std::vector<int> base;
    std::vector<char> kind;
    const int no = obstacle_ordinals(ncon, 5, type, count, CIRCLES, SPHERES, base, kind);
    CHECK(no == 9 && kind.size() == 9 && base.size() == 8);
    const int want_base[8] = {-1, 0, 2, -1, 5, -1, 6, 7};
    for (int i = 0; i < 8; i++) CHECK(base[i] == want_base[i]);
    const char want_kind[9] = {0, 0, 1, 1, 1, 1, 0, 0, 0};
    for (int j = 0; j < 9; j++) CHECK(kind[j] == want_kind[j]);
    CHECK(obs_width(no) == 36);

    // the table image: the same layout, a circle's third number stored as 0, everything else verbatim
    const long long B = 5;
    std::vector<double> obs(obs_width(no) * B);
    for (size_t i = 0; i < obs.size(); i++) obs[i] = 1.0 + (double)i;
    const std::vector<double> t = obstacle_table(obs.data(), kind, B);
    CHECK(t.size() == obs.size());
    for (long long b = 0; b < B; b++)
      for (int j = 0; j < no; j++)
        for (int q = 0; q < 4; q++) {
          const size_t i = ((size_t)b * no + j) * 4 + q;
          CHECK(t[i] == ((q == 2 && !kind[j]) ? 0.0 : obs[i]));
        }

    // multi-device split: B = 5 over parts of 3 and 2, every element of every slice read to its end
    const long long off[3] = {0, 3, 5};
    const size_t w = obs_width(no);
    for (int p = 0; p < 2; p++) {
      const double* s = part_slice(obs.data(), (size_t)off[p], w);
      const size_t cnt = (size_t)(off[p + 1] - off[p]) * w;
      const std::vector<double> tp = obstacle_table(s, kind, off[p + 1] - off[p]);
      CHECK(tp.size() == cnt);
      for (size_t i = 0; i < cnt; i++) CHECK(tp[i] == t[(size_t)off[p] * w + i]);
    }
    CHECK(part_slice(nullptr, 3, w) == nullptr);
  }

  // no obstacle constraint, an empty sets table, and a non-positive count
  {
    const int ncon[2] = {2, 1};
    const int type[3] = {BOUND, GOAL, CIRCLES};
    const int count[3] = {0, 3, 0};
    std::vector<int> base;
    std::vector<char> kind;
    CHECK(obstacle_ordinals(ncon, 1, type, count, CIRCLES, SPHERES, base, kind) == 0 && kind.empty());
    CHECK(base.size() == 2 && base[0] == -1 && base[1] == -1);
    CHECK(obstacle_ordinals(ncon, 2, type, count, CIRCLES, SPHERES, base, kind) == 0 && kind.empty());
    CHECK(base.size() == 3 && base[2] == 0);  // (a circles constraint without circles: an ordinal base, no ordinal)
    CHECK(obstacle_ordinals(nullptr, 0, nullptr, nullptr, CIRCLES, SPHERES, base, kind) == 0 && base.empty());
    CHECK(obstacle_table(nullptr, kind, 7).empty());
  }

  // error texts
  CHECK(obstacles_none_text().find("no circle or sphere") != std::string::npos);
  CHECK(obstacles_refuse_text().find("infeasible-start and minimum-time") != std::string::npos);
  const std::string s = obstacles_set_text("tog_refill");
  CHECK(s.rfind("tog_refill: per-trajectory obstacles are set", 0) == 0);
  CHECK(s.find("tog_set_trajectory_obstacles(h, NULL)") != std::string::npos);

  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
